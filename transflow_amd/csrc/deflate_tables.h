// RFC 1951's alphabets, stated once for the deflate coders (png.hip, flowzip.hip) and the decoder (flowunzip.hip).
// 3.2.5: length symbol 257 + k codes LENGTH_BASE[k] .. with LENGTH_EXTRA[k] extra bits, distance symbol k codes
// DIST_BASE[k] .. with DIST_EXTRA[k]; 3.2.7: the order in which a dynamic block sends the lengths of its code-length code.
#pragma once
#include <stdint.h>

namespace tf {
namespace deflate {

constexpr int N_SYMBOLS = 286, N_LENGTH_SYMBOLS = 29, END_OF_BLOCK = 256, MAX_MATCH = 258, MIN_MATCH = 3;
constexpr uint16_t LENGTH_BASE[29] = {
    3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258,
};
constexpr uint8_t LENGTH_EXTRA[29] = {
    0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0,
};
constexpr uint16_t DIST_BASE[30] = {
    1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
    193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577,
};
constexpr uint8_t DIST_EXTRA[30] = {
    0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13,
};
constexpr uint8_t CLEN_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

} // namespace deflate
} // namespace tf
