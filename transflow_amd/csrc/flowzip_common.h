// Flow archive members deflated on the device (flowzip.hip): the layout of the table buffer the table kernel writes and
// the other kernels read, the bound on a member's stream.
#pragma once
#include "common.h"
#include "crc32_common.h"
#include "deflate_tables.h"
#include "deflate_code.h"

namespace tf {
namespace flowzip {

using namespace deflate;

// distances as far as 64: the first twelve distance symbols
constexpr int MAX_DISTANCE = 64, N_DIST_SYMBOLS = 12;
static_assert(DIST_BASE[N_DIST_SYMBOLS - 1] + (1 << DIST_EXTRA[N_DIST_SYMBOLS - 1]) - 1 == MAX_DISTANCE,
              "the last distance symbol in use must end at MAX_DISTANCE");

// ---- the start of every coded band's block: BFINAL 0, BTYPE 10, HLIT 29, HDIST, HCLEN 15, nineteen 3-bit lengths of
// the code-length code (4 for the symbols 0 - 15, none for the repeat codes), then 286 + HDIST + 1 lengths of 4 bits
constexpr int HEADER_FIXED_BITS = 3 + 14 + 3 * 19;
constexpr int MAX_HEADER_BITS = HEADER_FIXED_BITS + 4 * (N_SYMBOLS + N_DIST_SYMBOLS);
constexpr int HEADER_WORDS = (MAX_HEADER_BITS + 31) / 32;

// ---- what k_fz_table writes for the member at hand
// an entry: (bits << 26) | value, the value as it goes into the stream from bit 0 (Huffman code reversed; a match's
// length bits above its code, the distance code's single 0 bit above them, the distance's extra bits on top: 25 bits
// at the most)
constexpr int ENTRY_SHIFT = 26;
constexpr uint32_t ENTRY_MASK = (1u << ENTRY_SHIFT) - 1;
struct Tables {
    uint32_t lit[END_OF_BLOCK + 1]; // the literals and end-of-block
    uint32_t match[MAX_MATCH + 1];  // [n], n = 3 .. 258
    uint32_t cost[N_SYMBOLS];       // the bits one occurrence of the symbol takes, a match's extra and distance bits included
    uint32_t header[HEADER_WORDS];  // stream bit 32 w + k in bit k of word w
    uint32_t header_bits;
    uint32_t repairs;               // how often the weights were halved to bring the code within 15 bits
    uint8_t lengths[N_SYMBOLS + 2];
};

// The LDS bit buffer of a wave holds the header or the 7 bits carried into a trip, what 64 lanes can OR into it per
// trip, and the band's end.  A lane's tokens per trip: two literals or one match, then its own literal or end-of-block.
constexpr int LANE_MAX_BITS = 64;
constexpr int LANE_WORST_BITS = 3 * MAX_CODE_BITS > MAX_CODE_BITS + 5 + 1 + 4 + MAX_CODE_BITS ? 3 * MAX_CODE_BITS
                                                                                              : 2 * MAX_CODE_BITS + 5 + 1 + 4;
constexpr int BIT_WORDS = (MAX_HEADER_BITS + 64 * LANE_MAX_BITS + 3 + 7 + 32) / 32 + 3;

// the stream of N bytes in bands of B: at most N + 5 per stored block + 5
inline uint64_t stream_bound(uint64_t N, uint64_t B)
{
    const uint64_t full = N / B, rest = N % B;
    return full * stored_bytes(B) + (rest ? stored_bytes(rest) : 0) + 5;
}

// band_bytes = 0 (Measured, has the sweep over 8, 16, 32 and 64 KB on 4K flows)
constexpr int DEFAULT_BAND_BYTES = 32768;
constexpr int MAX_PREFIX_BYTES = 4096;
constexpr uint32_t CODED_FLAG = 1u << 31; // in a band's size word: the band is coded, not stored

} // namespace flowzip
} // namespace tf
