// Baseline JPEG on the device (jpeg.hip): the tables of ITU-T T.81 Annex K, the layout of the table buffer the kernels
// read, and the bound on what an MCU can emit.
#pragma once
#include "common.h"

namespace tf {
namespace jpeg {

// ---- Annex K: K.1 quantisation tables (natural order), the zigzag sequence (position -> natural index), K.3 - K.6
// Huffman tables as DHT carries them: 16 counts, then the symbols.
constexpr uint8_t QUANT_LUMA[64] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99,
};

constexpr uint8_t QUANT_CHROMA[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
};

constexpr uint8_t ZIGZAG[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};

constexpr uint8_t DC_LUMA_BITS[16] = {
    0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0,
};

constexpr uint8_t DC_LUMA_VALS[12] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};

constexpr uint8_t DC_CHROMA_BITS[16] = {
    0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0,
};

constexpr uint8_t DC_CHROMA_VALS[12] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};

constexpr uint8_t AC_LUMA_BITS[16] = {
    0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125,
};

constexpr uint8_t AC_LUMA_VALS[162] = {
    1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113,
    20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114,
    130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55,
    56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
    90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
    132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
    164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
    196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
    227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250,
};

constexpr uint8_t AC_CHROMA_BITS[16] = {
    0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119,
};

constexpr uint8_t AC_CHROMA_VALS[162] = {
    0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34,
    50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209,
    10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54,
    55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88,
    89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122,
    130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
    162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
    194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
    226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250,
};

// ---- what the kernels read, in one device buffer of the handle
// a Huffman entry: (length << 16) | code; length 0 for a symbol the table does not have
struct Tables {
    uint32_t ac[2][256]; // [luma / chroma][run << 4 | size]
    uint32_t dc[2][16];  // [luma / chroma][size]
    uint16_t q8[2][64];  // 8 Q[k] in zigzag order: jfdctint's output is scaled by 8 (jcdctmgr.c)
    uint8_t zz[64];      // ZIGZAG
};

// ---- the bound.  A coded coefficient costs at most a 16-bit code and its value bits: 10 for an AC coefficient, 11 for
// a DC difference (8-bit samples: jchuff.c's MAX_COEF_BITS; the kernel clamps to them, which changes nothing libjpeg
// would not have refused).  A ZRL stands for 16 zero coefficients and an EOB for at least one, and both cost less than
// one coded coefficient, so a block costs at most 16 + 11 + 63 (16 + 10) = 1665 bits and an MCU of six blocks 9990.
// The interval is padded to a byte once, and every byte can be an 0xFF that takes an 0x00 after it.
// The bound assumes a 16-bit code for every symbol, so it holds for the frame's own tables (mode 1) as it stands.
constexpr int BLOCK_MAX_BITS = 16 + 11 + 63 * (16 + 10);

// ---- the chroma layouts, numbered as Pillow's `subsampling`.  An MCU is 8 x 8 pixels with blocks Y Cb Cr, 16 x 8 with
// Y0 Y1 Cb Cr, or 16 x 16 with Y00 Y01 Y10 Y11 Cb Cr.  The kernel codes a "trip" at a time: one 4:2:0 MCU, or two MCUs of
// the smaller layouts -- 6, 8 and 6 blocks, which keep the 48 or 64 lanes of the DCT passes busy.
enum Sampling { S444 = 0, S422 = 1, S420 = 2 };
constexpr int mcu_width(int sub) { return sub == S444 ? 8 : 16; }
constexpr int mcu_height(int sub) { return sub == S420 ? 16 : 8; }
constexpr int mcu_blocks(int sub) { return sub == S444 ? 3 : (sub == S422 ? 4 : 6); }
constexpr int trip_mcus(int sub) { return sub == S420 ? 1 : 2; }
constexpr int trip_blocks(int sub) { return mcu_blocks(sub) * trip_mcus(sub); }

constexpr int mcu_max_bits(int sub) { return mcu_blocks(sub) * BLOCK_MAX_BITS; }
inline size_t slot_bytes(int restart_mcus, int sub)
{
    const size_t bytes = ((size_t)restart_mcus * mcu_max_bits(sub) + 7) / 8; // with the padding
    return (2 * bytes + 3) & ~(size_t)3;                                     // stuffed; slots stay dword-aligned
}

// The LDS bit buffer of a wave holds one trip and the 7 bits carried into it.  It is sized for what 64 lanes can
// physically OR into it per block -- a lane's symbols are at most 64 bits, checked on the host when the tables are made
// -- not for the bound above: no data can make the kernel write outside it.
constexpr int LANE_MAX_BITS = 64;
constexpr int bit_words(int sub) { return (8 + trip_blocks(sub) * 64 * LANE_MAX_BITS) / 32 + 3; }
// With the frame's own tables nothing is checked on the host: ZRL may have a 16-bit code like any other symbol, and a
// lane's three ZRLs, its code and an 11-bit value come to 75 bits.  That kernel places a lane's bits as two pieces, the
// ZRLs (at most 48 bits) and the code with its value (at most 27), and its buffer is sized for 75.
constexpr int LANE_MAX_BITS_WIDE = 3 * 16 + 16 + 11;
constexpr int bit_words_wide(int sub) { return (8 + trip_blocks(sub) * 64 * LANE_MAX_BITS_WIDE) / 32 + 3; }

// ---- mode 1, the frame's own tables: what the gather pass counts and what k_jpeg_tables makes of it.  The four tables
// are in the order of the file's DHT segments: DC luma, AC luma, DC chroma, AC chroma.
constexpr int GATHER_COPIES = 8;
struct OwnTables {
    uint32_t counts[4][257]; // the histograms, summed by k_jpeg_tables; entry 256, the reserved symbol, is not counted
    uint32_t fault;          // bit t: table t has a code size above 32; bit 4 + t: table t has no symbol
    uint32_t pad;
    uint8_t bits[4][16];     // as DHT carries them
    uint8_t vals[4][256];    // the first sum(bits) of each are meant
    // what the gather pass adds to: interval i counts into copy i % GATHER_COPIES, so that fewer waves meet at one
    // counter (at 4K, 4050 waves add some 150 counters each)
    uint32_t partial[GATHER_COPIES][4][257];
};

} // namespace jpeg
} // namespace tf
