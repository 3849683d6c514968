// PNG on the device (png.hip): deflate's length alphabet, the layout of the table buffer the kernels read, and the
// bound on what a band can emit.
#pragma once
#include "common.h"

namespace tf {
namespace png {

// ---- RFC 1951 3.2.5: length symbol 257 + k codes LENGTH_BASE[k] .. with LENGTH_EXTRA[k] extra bits; 3.2.7: the order
// in which a dynamic block sends the lengths of its code-length code
constexpr int N_SYMBOLS = 286, N_LENGTH_SYMBOLS = 29, END_OF_BLOCK = 256, MAX_MATCH = 258, MIN_MATCH = 3;
constexpr uint16_t LENGTH_BASE[N_LENGTH_SYMBOLS] = {
    3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258,
};
constexpr uint8_t LENGTH_EXTRA[N_LENGTH_SYMBOLS] = {
    0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0,
};
constexpr uint8_t CLEN_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

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
    uint32_t crc[256];              // CRC-32, reflected, polynomial EDB88320
    uint32_t x2n[32];               // x^(2^k) mod the polynomial (zlib's x2n_table)
    uint32_t header[HEADER_WORDS];  // the HEADER_BITS above, stream bit 32 w + k in bit k of word w
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

// The LDS bit buffer of a wave holds the header or the 7 bits carried into a trip, what 64 lanes can physically OR into
// it per trip -- a lane's tokens are at most 64 bits, checked on the host when the table is made -- and the band's end.
// It is not sized by the bound above: no data can make the kernel write outside it.
constexpr int LANE_MAX_BITS = 64;
constexpr int BIT_WORDS = (HEADER_BITS + 64 * LANE_MAX_BITS + 3 + 7 + 32) / 32 + 3;

// the band of band_rows = 0 holds at least this much of the filtered stream
constexpr int DEFAULT_BAND_BYTES = 8192;

} // namespace png
} // namespace tf
