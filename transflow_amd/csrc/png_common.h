// PNG on the device (png.hip): the layout of the table buffer the kernels read, and the bound on what a band can emit.
#pragma once
#include "common.h"
#include "crc32_common.h"
#include "deflate_code.h"
#include "deflate_tables.h"

namespace tf {
namespace png {

using namespace deflate;

// ---- the constant start of every band's block: BFINAL 0, BTYPE 10, HLIT 29, HDIST 0, HCLEN 15, nineteen 3-bit lengths
// of the code-length code (4 for the symbols 0 - 15, none for the repeat codes), then 286 + 1 code lengths of 4 bits
constexpr int HEADER_BITS = 3 + 14 + 3 * 19 + 4 * (N_SYMBOLS + 1); // 1222
constexpr int HEADER_WORDS = (HEADER_BITS + 31) / 32;

// ---- what the kernels read, in one device buffer of the handle
// an entry: (bits << 24) | value, the value as it goes into the stream from bit 0 (Huffman code reversed; a match's
// extra bits above its code, and the distance code's single 0 bit above them)
struct Tables {
    uint32_t lit[END_OF_BLOCK + 1]; // the literals and end-of-block
    uint32_t match[MAX_MATCH + 1];  // [n], n = 3 .. 258
    Crc32Consts crc;                // (crc32_common.h)
    uint32_t header[HEADER_WORDS];  // the HEADER_BITS above, stream bit 32 w + k in bit k of word w
};

// ---- what k_png_table writes beside a Tables' entries and header when the code is the frame's own (tf_png_set_code)
struct FrameCode {
    uint32_t cost[N_SYMBOLS]; // the bits one occurrence of the symbol takes, a match's extra bits and distance bit included
    uint32_t repairs;         // how often the weights were halved to bring the code within 15 bits
    uint8_t lengths[N_SYMBOLS + 2];
};

// ---- the bound.  A band's data is the header, its bytes' tokens, end-of-block, the three bits of the empty stored
// block, at most 7 bits of padding and that block's four bytes.  A byte is coded as a literal, or as one of the n >= 3
// bytes of a match that costs its length code, at most 5 extra bits and the distance bit: the costliest coding of a
// byte is max(longest literal, max over n of ceil(match bits(n) / n)) =: byte_bits.
inline size_t slot_bytes(size_t band_bytes, int byte_bits, int eob_bits)
{
    const size_t bits = HEADER_BITS + band_bytes * (size_t)byte_bits + (size_t)eob_bits + 3 + 7 + 32;
    return (bits / 8 + 3) & ~(size_t)3; // slots stay dword-aligned
}
// With the frame's own code a band is coded only where that is smaller than stored_bytes(band_bytes), and that is below
// the bound above for any code whose longest literal has 8 bits or more (tf_png_set_code checks it for the handle's band).

// The LDS bit buffer of a wave holds the header or the 7 bits carried into a trip, what 64 lanes can physically OR into
// it per trip -- a lane's tokens are at most 64 bits, checked on the host when the table is made -- and the band's end.
// It is not sized by the bound above: no data can make the kernel write outside it.
constexpr int LANE_MAX_BITS = 64;
constexpr int BIT_WORDS = (HEADER_BITS + 64 * LANE_MAX_BITS + 3 + 7 + 32) / 32 + 3;

// the band of band_rows = 0 holds at least this much of the filtered stream
constexpr int DEFAULT_BAND_BYTES = 8192;

} // namespace png
} // namespace tf
