// Baseline JPEG of a device-resident RGB frame: what libjpeg writes for 8-bit YCbCr 4:2:0, one interleaved scan, the
// Annex K Huffman tables, jpeg_set_quality's tables and a restart interval -- byte for byte (tests/jpeg_ref.py is the
// numpy statement of the same rules, tests/golden/jpeg_*.npz are libjpeg's own files).
//
// Restart intervals are what make the entropy coder parallel: DC prediction starts over and the stream is byte-aligned
// at each, so an interval's bytes depend on nothing but its own MCUs.
//
//   k_jpeg_encode  one wave per interval.  Per MCU: lane l owns the 2 x 2 pixels under chroma sample l of the 16 x 16
//                  tile (the image's only read from HBM, 3 B/px), converts them (jccolor.c) and averages the chroma
//                  (jcsample.c h2v2_downsample); 48 lanes run jfdctint.c's row pass, then its column pass, on the six
//                  blocks in LDS; then block by block lane k takes zigzag coefficient k, quantises it (jcdctmgr.c), and
//                  a ballot of the non-zero lanes gives it its zero run, hence its symbols (jchuff.c encode_one_block:
//                  ZRLs, code, value bits; lane 0 the DC difference, lane 63 the EOB) -- a wave prefix sum of the bit
//                  counts places them and they are ORed into an LDS bit buffer.  After the MCU the whole bytes of that
//                  buffer go to the interval's staging slot, an 0x00 after every 0xFF (a ballot counts the 0xFFs
//                  before a lane's byte), and the bits left over are carried to the front.  The buffer is zeroed by
//                  the kernel before it is used and behind every flush.
//   k_slot_scan    exclusive sum of the intervals' byte counts, each with its marker's two (one work-group;
//                  stream_common.h).
//   k_jpeg_pack    one wave per interval copies its slot to its place in the packed stream and puts RSTn behind it, EOI
//                  behind the last; no byte at or past `capacity` is written.
//
// Mode 1 (tf_jpeg_set_optimize), the frame's own Huffman tables -- libjpeg's optimize_coding, Pillow's optimize=True,
// byte for byte (tests/jpeg_ref.py, tests/golden/jpegopt_*.npz).  k_jpeg_encode is a template over its pass:
//   k_jpeg_encode<GATHER>     the same front; in place of placing bits the lanes count their symbols (jchuff.c
//                             encode_mcu_gather) into an LDS histogram of the wave, added to the frame's at the end.
//   k_jpeg_tables             one work-group, a wave per table: jpeg_gen_optimal_table's rule (jpeg_huff.h) -> the DHT
//                             form for the header, the entries for a second Tables, a fault word.
//   k_jpeg_encode<EMIT_WIDE>  the emit pass with those tables; a lane's symbols may take 75 bits and go in two pieces.
// The scan of lengths and the pack are the same; the header is made on the host from the DHT form, per frame.
//
// Dummy blocks (jccoefct.c compress_data): the luma blocks of an MCU beyond ceil(W / 8) x ceil(H / 8) are not made
// from pixels; their AC coefficients are zero and their DC is that of the block coded before them.
// Chroma rows (jcprepct.c pre_process_data): the input is padded to an even row count only, and the DOWNSAMPLED plane
// is then padded with its last row -- a chroma row below the image averages rows H - 2 and H - 1 of an image of even
// height, not H - 1 twice.
//
// The other chroma layouts (tf_jpeg_create_sub; tests/jpeg_ref.py, tests/golden/jpegsub_*.npz): k_jpeg_encode is a
// template over the layout too.  4:4:4: an MCU is 8 x 8 pixels, blocks Y Cb Cr, the chroma samples as converted, no
// dummy blocks.  4:2:2: 16 x 8 pixels, blocks Y0 Y1 Cb Cr, chroma by jcsample.c h2v1_downsample -- (a + b + bias) >> 1,
// bias 0, 1, 0, 1 ... along the output row -- and Y1 a dummy in the last MCU column when ceil(W / 8) is odd.  Edges are
// replicated samples, which is the clamp of the pixel's coordinates.  Only SOF0's luma sampling byte tells the files
// apart: 0x11, 0x21, 0x22.
#include "jpeg_common.h"
#include "jpeg_huff.h"
#include "stream_common.h"

#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace tf {
namespace jpeg {

// jfdctint.c (CONST_BITS 13, PASS1_BITS 2)
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
              FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
              FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jpeg_fdct_islow over 8 values `stride` apart
template <bool FIRST> __device__ __forceinline__ void fdct_pass(int *d, int stride)
{
    int v[8];
#pragma unroll
    for (int i = 0; i < 8; i++)
        v[i] = d[i * stride];
    int tmp0 = v[0] + v[7], tmp7 = v[0] - v[7], tmp1 = v[1] + v[6], tmp6 = v[1] - v[6];
    int tmp2 = v[2] + v[5], tmp5 = v[2] - v[5], tmp3 = v[3] + v[4], tmp4 = v[3] - v[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int N = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    if (FIRST) {
        d[0] = (tmp10 + tmp11) << PASS1_BITS;
        d[4 * stride] = (tmp10 - tmp11) << PASS1_BITS;
    } else {
        d[0] = descale(tmp10 + tmp11, PASS1_BITS);
        d[4 * stride] = descale(tmp10 - tmp11, PASS1_BITS);
    }
    int z1 = (tmp12 + tmp13) * FIX_0_541196100;
    d[2 * stride] = descale(z1 + tmp13 * FIX_0_765366865, N);
    d[6 * stride] = descale(z1 + tmp12 * (-FIX_1_847759065), N);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    tmp4 *= FIX_0_298631336, tmp5 *= FIX_2_053119869, tmp6 *= FIX_3_072711026, tmp7 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223, z2 *= -FIX_2_562915447, z3 *= -FIX_1_961570560, z4 *= -FIX_0_390180644;
    z3 += z5, z4 += z5;
    d[7 * stride] = descale(tmp4 + z1 + z3, N);
    d[5 * stride] = descale(tmp5 + z2 + z4, N);
    d[3 * stride] = descale(tmp6 + z2 + z3, N);
    d[1 * stride] = descale(tmp7 + z1 + z4, N);
}

struct Px {
    int r, g, b;
};

__device__ __forceinline__ Px load_px(const uint8_t *__restrict__ rgb, int W, int y, int x)
{
    const uint8_t *p = rgb + ((size_t)y * W + x) * 3;
    return Px{p[0], p[1], p[2]};
}

// jccolor.c rgb_ycc_convert, SCALEBITS 16
__device__ __forceinline__ int ycc_y(Px p) { return (19595 * p.r + 38470 * p.g + 7471 * p.b + 32768) >> 16; }
__device__ __forceinline__ int ycc_cb(Px p) { return (-11059 * p.r - 21709 * p.g + 32768 * p.b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int ycc_cr(Px p) { return (32768 * p.r - 27439 * p.g - 5329 * p.b + (128 << 16) + 32767) >> 16; }

struct EncodeArgs {
    const uint8_t *rgb;
    int W, H;
    int mcus_x, n_mcus, restart_mcus;
    int lum_bx, lum_by;   // the luma block grid: ceil(W / 8) x ceil(H / 8)
    int chroma_rows;      // ceil(H / 2): the downsampled rows that come from pixels
    const Tables *tables;
    uint8_t *staging;     // n_intervals slots of slot_bytes
    uint32_t slot_bytes;
    uint32_t *lengths;    // per interval: the bytes it wrote
    uint32_t *overflow;   // set if an interval had more bytes than its slot (the bound of jpeg_common.h says: never)
    uint32_t *counts;     // GATHER: the frame's histograms, OwnTables::partial
};

// `len` bits (1 to 64), right-aligned in `bits`, ORed into the bit buffer at bit `p`; nothing outside WORDS words
template <int WORDS> __device__ __forceinline__ void place_bits(uint32_t *s_bits, uint32_t p, unsigned long long bits, int len)
{
    const unsigned long long w = bits << (64 - len);
    const uint32_t word = p >> 5, sh = p & 31;
    const uint32_t w0 = (uint32_t)(w >> 32 >> sh), w1 = (uint32_t)(w >> sh);
    const uint32_t w2 = sh ? (uint32_t)(w << (32 - sh)) : 0u;
    if (word + 2 < WORDS) {
        if (w0)
            atomicOr(&s_bits[word], w0);
        if (w1)
            atomicOr(&s_bits[word + 1], w1);
        if (w2)
            atomicOr(&s_bits[word + 2], w2);
    }
}

// One kernel, three passes: EMIT codes with tables whose lanes the host has checked to fit 64 bits (Annex K's);
// GATHER runs the same front and counts the symbols EMIT would write, into an LDS histogram of the wave whose non-zero
// counters are added to the frame's when the interval is done (jchuff.c encode_mcu_gather); EMIT_WIDE codes with
// tables made on the device (k_jpeg_tables), where a lane's symbols may take 75 bits.
enum Pass { EMIT = 0, GATHER = 1, EMIT_WIDE = 2 };

// SUB is the chroma layout.  A trip of the MCU loop codes one 4:2:0 MCU, or two MCUs of 4:4:4 or 4:2:2 (the second may
// lie at the start of the next MCU row; an interval of an odd count ends with a trip of one): block b of the trip is
// block b % BPM of MCU b / BPM, the stages run once per trip, and the bits are flushed once per trip.
template <int PASS, int SUB> __global__ __launch_bounds__(WAVE) void k_jpeg_encode(const EncodeArgs a, const FastDiv div_mcus_x)
{
    constexpr int BPM = mcu_blocks(SUB), TRIP = trip_mcus(SUB), NB = trip_blocks(SUB);
    constexpr int WORDS = PASS == EMIT_WIDE ? bit_words_wide(SUB) : (PASS == GATHER ? 1 : bit_words(SUB));
    constexpr int HIST = PASS == GATHER ? 4 * 256 : 1;
    __shared__ int s_blk[NB][64];         // samples - 128, then coefficients: the trip's blocks in coding order
    __shared__ uint32_t s_bits[WORDS];    // the trip's bits, first bit of the stream in bit 31 of word 0
    __shared__ uint32_t s_hist[HIST];     // GATHER: [DC luma, AC luma, DC chroma, AC chroma][symbol]
    const int lane = threadIdx.x;
    const Tables &t = *a.tables;
    const int q_luma = t.q8[0][lane], q_chroma = t.q8[1][lane], zz = t.zz[lane];
    for (int w = lane; w < WORDS; w += WAVE)
        s_bits[w] = 0;
    for (int w = lane; w < HIST; w += WAVE)
        s_hist[w] = 0;
    const int first = blockIdx.x * a.restart_mcus; // (n_intervals * restart_mcus < n_mcus + restart_mcus <= 2^25)
    const int last = min(first + a.restart_mcus, a.n_mcus);
    uint8_t *slot = a.staging + (size_t)blockIdx.x * a.slot_bytes;
    int last_dc[3] = {0, 0, 0};
    uint32_t bitpos = 0; // bits in s_bits
    uint32_t outpos = 0; // bytes in the slot
    const int cy = lane >> 3, cx = lane & 7;
    __syncthreads();
    for (int m = first; m < last; m += TRIP) {
        const int my = (int)fast_div((uint32_t)m, div_mcus_x), mx = m - my * a.mcus_x;
        const bool two = TRIP == 2 && m + 1 < last;                 // the trip has its second MCU (wave-uniform)
        const int mx1 = mx + 1 < a.mcus_x ? mx + 1 : 0, my1 = mx + 1 < a.mcus_x ? my : my + 1; // where that one is
        // ---- colour, downsample
        if constexpr (SUB == S444) { // lane l owns pixel l of each MCU; the edges are replicated samples
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (k == 1 && !two)
                    break;
                const int x = min((k ? mx1 : mx) * 8 + cx, a.W - 1), y = min((k ? my1 : my) * 8 + cy, a.H - 1);
                const Px p = load_px(a.rgb, a.W, y, x);
                s_blk[3 * k][lane] = ycc_y(p) - 128;
                s_blk[3 * k + 1][lane] = ycc_cb(p) - 128;
                s_blk[3 * k + 2][lane] = ycc_cr(p) - 128;
            }
        } else if constexpr (SUB == S422) { // lane l owns the 2 x 1 pixels under chroma sample l of each MCU
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (k == 1 && !two)
                    break;
                const int xb = (k ? mx1 : mx) * 16 + 2 * cx, y = min((k ? my1 : my) * 8 + cy, a.H - 1);
                const Px p0 = load_px(a.rgb, a.W, y, min(xb, a.W - 1)), p1 = load_px(a.rgb, a.W, y, min(xb + 1, a.W - 1));
                int *yb = &s_blk[4 * k + (cx >> 2)][cy * 8 + ((2 * cx) & 7)];
                yb[0] = ycc_y(p0) - 128, yb[1] = ycc_y(p1) - 128;
                const int bias = cx & 1; // 0, 1, 0, 1 ... along the output row (jcsample.c h2v1_downsample)
                s_blk[4 * k + 2][lane] = ((ycc_cb(p0) + ycc_cb(p1) + bias) >> 1) - 128;
                s_blk[4 * k + 3][lane] = ((ycc_cr(p0) + ycc_cr(p1) + bias) >> 1) - 128;
            }
        } else {
            const int x0 = min(mx * 16 + 2 * cx, a.W - 1), x1 = min(mx * 16 + 2 * cx + 1, a.W - 1);
            const int y0 = min(my * 16 + 2 * cy, a.H - 1), y1 = min(my * 16 + 2 * cy + 1, a.H - 1);
            Px p00 = load_px(a.rgb, a.W, y0, x0), p01 = load_px(a.rgb, a.W, y0, x1);
            Px p10 = load_px(a.rgb, a.W, y1, x0), p11 = load_px(a.rgb, a.W, y1, x1);
            int *yb = &s_blk[(cy >> 2) * 2 + (cx >> 2)][((2 * cy) & 7) * 8 + ((2 * cx) & 7)];
            yb[0] = ycc_y(p00) - 128, yb[1] = ycc_y(p01) - 128, yb[8] = ycc_y(p10) - 128, yb[9] = ycc_y(p11) - 128;
            const int cr = min(my * 8 + cy, a.chroma_rows - 1); // below the image: the last downsampled row again
            const int c0 = min(2 * cr, a.H - 1), c1 = min(2 * cr + 1, a.H - 1);
            if (c0 != y0 || c1 != y1) {
                p00 = load_px(a.rgb, a.W, c0, x0), p01 = load_px(a.rgb, a.W, c0, x1);
                p10 = load_px(a.rgb, a.W, c1, x0), p11 = load_px(a.rgb, a.W, c1, x1);
            }
            const int bias = 1 + (cx & 1); // 1, 2, 1, 2 ... along the output row (an MCU starts at an even column)
            s_blk[4][lane] = ((ycc_cb(p00) + ycc_cb(p01) + ycc_cb(p10) + ycc_cb(p11) + bias) >> 2) - 128;
            s_blk[5][lane] = ((ycc_cr(p00) + ycc_cr(p01) + ycc_cr(p10) + ycc_cr(p11) + bias) >> 2) - 128;
        }
        __syncthreads();
        // ---- DCT: rows, then columns
        const int dct_lanes = 8 * (TRIP == 1 || two ? NB : BPM);
        if (lane < dct_lanes)
            fdct_pass<true>(&s_blk[lane >> 3][(lane & 7) * 8], 1);
        __syncthreads();
        if (lane < dct_lanes)
            fdct_pass<false>(&s_blk[lane >> 3][lane & 7], 8);
        __syncthreads();
        // ---- quantise and code, block by block
        int prev_dc = 0;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            if (TRIP == 2 && b >= BPM && !two)
                break;
            const int bi = b % BPM, n_luma = BPM - 2; // the block within its MCU; the luma blocks come first
            const int comp = bi < n_luma ? 0 : bi - n_luma + 1, tb = bi < n_luma ? 0 : 1;
            const int c = s_blk[b][zz];
            const uint32_t q8 = (uint32_t)(tb ? q_chroma : q_luma);
            const uint32_t mag = ((uint32_t)abs(c) + (q8 >> 1)) / q8;
            int v = c < 0 ? -(int)mag : (int)mag;
            bool dummy = false; // (4:4:4 has none; 4:2:2 only the second luma block, in the last MCU column)
            if (SUB == S420)
                dummy = b > 0 && b < 4 && (2 * mx + (b & 1) >= a.lum_bx || 2 * my + (b >> 1) >= a.lum_by);
            else if (SUB == S422)
                dummy = bi == 1 && 2 * (b < BPM ? mx : mx1) + 1 >= a.lum_bx;
            if (dummy)
                v = lane == 0 ? prev_dc : 0;
            if (lane > 0)
                v = max(-1023, min(1023, v)); // (never: an AC coefficient of 8-bit samples has 10 bits)
            const int dc = __builtin_amdgcn_readfirstlane(v);
            prev_dc = dc;
            const unsigned long long nonzero = __ballot(v != 0) & ~1ull; // the AC lanes
            int sym_v = v;
            int symbol = -1; // what the lane's value is coded with: 0 .. 255 in the AC table, 256 + category in the DC table
            int n_zrl = 0;
            if (lane == 0) {
                sym_v = max(-2047, min(2047, dc - last_dc[comp]));
                symbol = 256 + 32 - __clz(abs(sym_v));
            } else if (v != 0) {
                const unsigned long long below = nonzero & ((1ull << lane) - 1);
                const int prev = below ? 63 - __clzll((long long)below) : 0;
                const int run = lane - 1 - prev;
                n_zrl = run >> 4;
                symbol = ((run & 15) << 4) | (32 - __clz(abs(v)));
            } else if (lane == 63) {
                symbol = 0x00; // EOB: the block ends in zeros
            }
            last_dc[comp] = dc;
            if constexpr (PASS == GATHER) {
                uint32_t *dc_hist = &s_hist[(2 * tb) * 256], *ac_hist = &s_hist[(2 * tb + 1) * 256];
                if (symbol >= 256)
                    atomicAdd(&dc_hist[symbol - 256], 1u);
                else if (symbol >= 0)
                    atomicAdd(&ac_hist[symbol], 1u);
                if (n_zrl)
                    atomicAdd(&ac_hist[0xF0], (uint32_t)n_zrl);
                continue;
            }
            const uint32_t entry = symbol < 0 ? 0u : (symbol >= 256 ? t.dc[tb][symbol - 256] : t.ac[tb][symbol]);
            const int nbits = sym_v == 0 ? 0 : 32 - __clz(abs(sym_v));
            const uint32_t value = (uint32_t)(sym_v < 0 ? sym_v - 1 : sym_v) & ((1u << nbits) - 1);
            unsigned long long bits = 0;
            int len = 0;
            if constexpr (PASS == EMIT) {
                if (n_zrl) {
                    const uint32_t zrl = t.ac[tb][0xF0];
                    for (int i = 0; i < n_zrl; i++)
                        bits = (bits << (zrl >> 16)) | (zrl & 0xFFFF), len += zrl >> 16;
                }
                bits = (bits << (entry >> 16)) | (entry & 0xFFFF), len += entry >> 16;
                bits = (bits << nbits) | value, len += nbits;
                len = min(len, LANE_MAX_BITS); // (never: the host checked the tables)
                const int incl = wave_inclusive_sum(len, lane);
                if (len)
                    place_bits<WORDS>(s_bits, bitpos + (uint32_t)(incl - len), bits, len);
                bitpos += (uint32_t)__shfl(incl, WAVE - 1, WAVE);
            } else { // two pieces: the ZRLs, then the code with its value
                if (n_zrl) {
                    const uint32_t zrl = t.ac[tb][0xF0];
                    const int zl = min((int)(zrl >> 16), 16); // (never more: k_jpeg_tables limits to 16)
                    for (int i = 0; i < min(n_zrl, 3); i++)
                        bits = (bits << zl) | (zrl & 0xFFFF), len += zl;
                }
                const int el = min((int)(entry >> 16), 16);
                const unsigned long long tail = ((unsigned long long)(entry & 0xFFFF) << nbits) | value;
                const int tail_len = el + nbits; // at most 27
                const int incl = wave_inclusive_sum(len + tail_len, lane);
                const uint32_t p = bitpos + (uint32_t)(incl - len - tail_len);
                if (len)
                    place_bits<WORDS>(s_bits, p, bits, len);
                if (tail_len)
                    place_bits<WORDS>(s_bits, p + (uint32_t)len, tail, tail_len);
                bitpos += (uint32_t)__shfl(incl, WAVE - 1, WAVE);
            }
        }
        if constexpr (PASS == GATHER) {
            __syncthreads(); // s_blk is the next MCU's
            continue;        // nothing to flush
        }
        // ---- the trip's whole bytes to the slot; the interval's last trip pads with ones first (flush_bits)
        if (m + TRIP >= last && (bitpos & 7)) {
            const uint32_t pad = 8 - (bitpos & 7);
            if (lane == 0)
                atomicOr(&s_bits[bitpos >> 5], ((1u << pad) - 1) << (32 - (bitpos & 31) - pad));
            bitpos += pad;
        }
        __syncthreads();
        const uint32_t n_bytes = bitpos >> 3;
        for (uint32_t base = 0; base < n_bytes; base += WAVE) {
            const uint32_t j = base + lane;
            const bool valid = j < n_bytes;
            const uint32_t byte = valid ? (s_bits[j >> 2] >> (24 - 8 * (j & 3))) & 0xFF : 0;
            const unsigned long long ff = __ballot(valid && byte == 0xFF);
            const uint32_t pos = outpos + lane + __popcll(ff & ((1ull << lane) - 1));
            if (valid) {
                if (pos < a.slot_bytes)
                    slot[pos] = (uint8_t)byte;
                if (byte == 0xFF && pos + 1 < a.slot_bytes)
                    slot[pos + 1] = 0;
            }
            outpos += min((uint32_t)WAVE, n_bytes - base) + __popcll(ff);
        }
        // ---- the bits left over go to the front of a zeroed buffer
        const uint32_t rem = bitpos & 7;
        const uint32_t carry = rem ? ((s_bits[n_bytes >> 2] >> (24 - 8 * (n_bytes & 3))) & 0xFF) << 24 : 0;
        const uint32_t used = (bitpos >> 5) + 3;
        __syncthreads();
        for (uint32_t w = lane; w < used && w < WORDS; w += WAVE)
            s_bits[w] = w == 0 ? carry : 0;
        bitpos = rem;
        __syncthreads();
    }
    if constexpr (PASS == GATHER) {
        __syncthreads();
        uint32_t *counts = a.counts + (size_t)(blockIdx.x % GATHER_COPIES) * (4 * 257);
        for (int i = lane; i < HIST; i += WAVE)
            if (const uint32_t n = s_hist[i])
                atomicAdd(&counts[(i >> 8) * 257 + (i & 255)], n);
        return;
    }
    if (lane == 0) {
        a.lengths[blockIdx.x] = min(outpos, a.slot_bytes);
        if (outpos > a.slot_bytes)
            *a.overflow = 1;
    }
}

// The four tables of the frame from its histograms: wave t makes table t (jpeg_huff.h has the rule).  With WAVE_PICK
// the lanes hold the 257 frequencies in registers, five each, and one wave reduction per merge finds the two smallest
// keys (frequency, -index): libjpeg's c1, and c2, "the same choice over the rest".  The trees are not chained: every
// lane keeps, for each of its symbols, the index its tree goes by (c1 survives a merge, c2's tree takes c1's) and its
// code size, one more for every merge its tree is part of -- what libjpeg's walk along the `others` chains adds up.
// The wave then finishes as huff_finish does.  Without WAVE_PICK lane 0 runs gen_optimal_table as the host does: the
// form the other is measured against and tested equal to.
// Writes the DHT form to `own`, the entries to the frame's Tables, and own->fault.
constexpr int TABLES_BLOCK = 4 * WAVE;

struct TwoKeys {
    unsigned long long k1, k2; // the smallest and the second smallest
};

__device__ __forceinline__ void two_keys_add(TwoKeys &t, unsigned long long k)
{
    const unsigned long long lo = k < t.k1 ? k : t.k1, hi = k < t.k1 ? t.k1 : k;
    t.k1 = lo, t.k2 = hi < t.k2 ? hi : t.k2;
}

// the keys of lane (l ^ 1), (l ^ 2), then of the mirrored lane of 8 and of 16: data-parallel moves within a row of 16
// lanes, which cost an ALU instruction where a shuffle goes through the LDS crossbar
template <int CTRL> __device__ __forceinline__ unsigned long long row_move(unsigned long long v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}

template <int CTRL> __device__ __forceinline__ void two_keys_row_step(TwoKeys &t)
{
    const unsigned long long a = row_move<CTRL>(t.k1), b = row_move<CTRL>(t.k2);
    two_keys_add(t, a); // (the two lanes hold different keys, or NONE)
    two_keys_add(t, b);
}

__device__ __forceinline__ TwoKeys wave_two_smallest(TwoKeys t)
{
    two_keys_row_step<0xB1>(t);  // quad_perm [1, 0, 3, 2]
    two_keys_row_step<0x4E>(t);  // quad_perm [2, 3, 0, 1]
    two_keys_row_step<0x141>(t); // row_half_mirror: the other quad of the eight
    two_keys_row_step<0x140>(t); // row_mirror: the other eight of the row
#pragma unroll
    for (int o = 16; o < WAVE; o <<= 1) {
        const unsigned long long a = __shfl_xor(t.k1, o, WAVE), b = __shfl_xor(t.k2, o, WAVE);
        two_keys_add(t, a);
        two_keys_add(t, b);
    }
    return t;
}

template <bool WAVE_PICK> __global__ __launch_bounds__(TABLES_BLOCK) void k_jpeg_tables(OwnTables *own, Tables *tables)
{
    __shared__ HuffWork s_work[4];
    __shared__ uint8_t s_bits16[4][16], s_vals[4][256];
    __shared__ int s_count[4][HUFF_MAX_CLEN + 2]; // WAVE_PICK: the symbols of every code size
    const int t = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    HuffWork &w = s_work[t];
    uint32_t *counts = own->counts[t];
    int fault = HUFF_OK, n_vals = 0;
    for (int i = lane; i < 256; i += WAVE) {
        s_vals[t][i] = 0;
        uint32_t n = 0;
        for (int c = 0; c < GATHER_COPIES; c++)
            n += own->partial[c][t][i];
        counts[i] = n;
    }
    __syncthreads();
    if (!WAVE_PICK) {
        for (int i = lane; i < 256; i += WAVE)
            w.freq[i] = counts[i];
        __syncthreads();
        if (lane == 0)
            fault = gen_optimal_table(w, s_bits16[t], s_vals[t], &n_vals);
    } else {
        constexpr unsigned long long NONE = ~0ull;
        // symbols lane, lane + 64 ...; the reserved symbol 256 is lane 0's fifth
        uint32_t f[5];
        int tree[5], size[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int i = lane + WAVE * k;
            f[k] = i < 256 ? counts[i] : (i == 256 ? 1u : 0u);
            tree[k] = i, size[k] = 0;
        }
        for (;;) {
            TwoKeys two{NONE, NONE};
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const int i = lane + WAVE * k;
                if (f[k] && f[k] <= HUFF_SENTINEL && i < HUFF_SYMS)
                    two_keys_add(two, ((unsigned long long)f[k] << 32) | (uint32_t)(256 - i)); // smallest frequency, largest index
            }
            two = wave_two_smallest(two);
            if (two.k2 == NONE)
                break;
            const int c1 = 256 - (int)(uint32_t)two.k1, c2 = 256 - (int)(uint32_t)two.k2;
            const uint32_t sum = (uint32_t)(two.k1 >> 32) + (uint32_t)(two.k2 >> 32);
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const int i = lane + WAVE * k;
                f[k] = i == c1 ? sum : (i == c2 ? 0u : f[k]);
                const bool in1 = tree[k] == c1, in2 = tree[k] == c2;
                size[k] += (in1 || in2) && size[k] < 0xFFFF;
                tree[k] = in2 ? c1 : tree[k];
            }
        }
        // huff_finish, by the wave: the counts per size with LDS atomics, a symbol's place among the values by counting
        // the symbols before it in (code size, symbol) order; lane 0 limits the sizes
        bool over = false, used = false;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int i = lane + WAVE * k;
            if (i < HUFF_SYMS)
                w.codesize[i] = (uint16_t)size[k];
            over |= i < HUFF_SYMS && size[k] > HUFF_MAX_CLEN;
            used |= i < 256 && size[k] > 0;
        }
        if (lane < HUFF_MAX_CLEN + 2)
            s_count[t][lane] = 0;
        __syncthreads();
        fault = __ballot(over) ? HUFF_CLEN_OVERFLOW : (__ballot(used) ? HUFF_OK : HUFF_EMPTY);
        if (fault == HUFF_OK) {
#pragma unroll
            for (int k = 0; k < 5; k++)
                if (lane + WAVE * k < HUFF_SYMS && size[k])
                    atomicAdd(&s_count[t][size[k]], 1);
            int before[4] = {0, 0, 0, 0};
            for (int j = 0; j < 256; j++) {
                const int sj = w.codesize[j];
#pragma unroll
                for (int k = 0; k < 4; k++)
                    before[k] += sj && (sj < size[k] || (sj == size[k] && j < lane + WAVE * k));
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (size[k])
                    s_vals[t][before[k] & 255] = (uint8_t)(lane + WAVE * k);
        }
        __syncthreads();
        if (lane == 0 && fault == HUFF_OK)
            huff_limit(s_count[t], s_bits16[t]);
    }
    if (lane == 0) {
        if (fault != HUFF_OK) {
            atomicOr(&own->fault, 1u << (fault == HUFF_CLEN_OVERFLOW ? t : 4 + t));
            for (int i = 0; i < 16; i++)
                s_bits16[t][i] = 0; // no code: the emit pass then writes nothing with this table
        }
        huff_entries(s_bits16[t], s_vals[t], t & 1 ? tables->ac[t >> 1] : tables->dc[t >> 1], t & 1 ? 256 : 16);
    }
    __syncthreads();
    for (int i = lane; i < 256; i += WAVE)
        own->vals[t][i] = s_vals[t][i];
    if (lane < 16)
        own->bits[t][lane] = s_bits16[t][lane];
}

// interval i: its bytes to out + offsets[i] (the markers before it are counted in), then FF D0+(i mod 8), or FF D9
// behind the last one
constexpr int PACK_BLOCK = 256;
__global__ __launch_bounds__(PACK_BLOCK) void k_jpeg_pack(const uint8_t *__restrict__ staging, uint32_t slot_bytes,
                                                          const uint32_t *__restrict__ lengths, const uint32_t *__restrict__ offsets,
                                                          int n, uint8_t *__restrict__ out, size_t capacity)
{
    const int i = blockIdx.x * (PACK_BLOCK / WAVE) + threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (i >= n)
        return;
    const uint8_t *src = staging + (size_t)i * slot_bytes;
    const uint32_t len = min(lengths[i], slot_bytes);
    const size_t dst = (size_t)offsets[i];
    for (uint32_t j = lane; j < len; j += WAVE)
        if (dst + j < capacity)
            out[dst + j] = src[j];
    if (lane < 2 && dst + len + lane < capacity)
        out[dst + len + lane] = lane == 0 ? 0xFF : (i == n - 1 ? 0xD9 : 0xD0 + (i & 7));
}

// ---- host: tables and header ----------------------------------------------------------------------------------------
// jcparam.c jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)
static void quant_table(const uint8_t *base, int quality, uint8_t *out /*natural order*/)
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; k++) {
        const long v = ((long)base[k] * scale + 50) / 100;
        out[k] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

static void put_segment(std::vector<uint8_t> &out, int marker, const std::vector<uint8_t> &payload)
{
    const size_t n = payload.size() + 2;
    out.push_back(0xFF), out.push_back((uint8_t)marker), out.push_back((uint8_t)(n >> 8)), out.push_back((uint8_t)n);
    out.insert(out.end(), payload.begin(), payload.end());
}

static void put_dht(std::vector<uint8_t> &out, int tc_th, const uint8_t *bits, const uint8_t *vals)
{
    std::vector<uint8_t> p{(uint8_t)tc_th};
    int n = 0;
    for (int i = 0; i < 16; i++)
        p.push_back(bits[i]), n += bits[i];
    p.insert(p.end(), vals, vals + n);
    put_segment(out, 0xC4, p);
}

// jcmarker.c: write_file_header, write_frame_header, write_scan_header
struct Dht {
    const uint8_t *bits, *vals;
};
static const Dht ANNEX_K[4] = {{DC_LUMA_BITS, DC_LUMA_VALS}, {AC_LUMA_BITS, AC_LUMA_VALS}, {DC_CHROMA_BITS, DC_CHROMA_VALS},
                               {AC_CHROMA_BITS, AC_CHROMA_VALS}};

static std::vector<uint8_t> make_header(int H, int W, const uint8_t q[2][64], int restart_mcus, int sub, const Dht *dht = ANNEX_K)
{
    const uint8_t luma_sampling = (uint8_t)((mcu_width(sub) / 8) << 4 | (mcu_height(sub) / 8)); // 0x11, 0x21, 0x22
    std::vector<uint8_t> out{0xFF, 0xD8};
    put_segment(out, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int n = 0; n < 2; n++) {
        std::vector<uint8_t> p{(uint8_t)n};
        for (int k = 0; k < 64; k++)
            p.push_back(q[n][ZIGZAG[k]]);
        put_segment(out, 0xDB, p);
    }
    put_segment(out, 0xC0, {8, (uint8_t)(H >> 8), (uint8_t)H, (uint8_t)(W >> 8), (uint8_t)W, 3, 1, luma_sampling, 0, 2, 0x11, 1, 3,
                            0x11, 1});
    put_dht(out, 0x00, dht[0].bits, dht[0].vals);
    put_dht(out, 0x10, dht[1].bits, dht[1].vals);
    put_dht(out, 0x01, dht[2].bits, dht[2].vals);
    put_dht(out, 0x11, dht[3].bits, dht[3].vals);
    put_segment(out, 0xDD, {(uint8_t)(restart_mcus >> 8), (uint8_t)restart_mcus});
    put_segment(out, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return out;
}

} // namespace jpeg
} // namespace tf

using namespace tf;
using namespace tf::jpeg;

// restart_mcus = 0: the fastest interval whose file is within 2 % of the smallest of the sweep 1, 2, 4, 8, 16, an MCU
// row, at 4K and at 1080p alike (tools/bench_jpeg.py, profiles/jpeg_bench.json; DESIGN.md section 15 has the table).
// Shorter intervals pay in markers and restarted DC prediction, longer ones in waves that code more MCUs one by one.
static constexpr int DEFAULT_RESTART_MCUS = 8;
// The other layouts keep that interval's 48 blocks: 16 MCUs of three, 12 of four.  Not tuned: tools/bench_jpeg_subsampling.py
// measures them beside half and twice as many.
static constexpr int default_restart_mcus(int sub) { return DEFAULT_RESTART_MCUS * mcu_blocks(S420) / mcu_blocks(sub); }
static_assert(default_restart_mcus(S444) == 16 && default_restart_mcus(S422) == 12 && default_restart_mcus(S420) == 8, "48 blocks");

struct tf_jpeg {
    int H = 0, W = 0, quality = 0, restart_mcus = 0;
    int sub = S420; // the chroma layout: a Sampling
    int mcus_x = 0, n_mcus = 0, n_intervals = 0;
    std::vector<uint8_t> header;
    DevBuf tables, upload;
    SlotStream s; // a slot an interval; packed, the scan: the intervals with a marker behind each
    // mode 1, the frame's own tables (tf_jpeg_set_optimize); the buffers are allocated by the first call that needs them
    int optimize = 0;
    uint8_t q[2][64];                        // the quantisation tables, natural order: a header is made per frame
    DevBuf own, own_tables;                  // OwnTables; the Tables the emit pass reads (tables' copy, own entries)
    PinnedBuf own_host;                      // OwnTables' fault, bits and vals, as the last encode left them
    std::vector<uint8_t> own_header;         // the header of the last mode 1 encode; empty: none
    bool one_lane_tables = false;            // TF_JPEG_TABLES_ONE_LANE=1: k_jpeg_tables without its wave reductions, to measure
    const std::vector<uint8_t> &file_header() const { return optimize ? own_header : header; }
};

static const char *const TABLE_NAMES[4] = {"DC luma", "AC luma", "DC chroma", "AC chroma"};
constexpr size_t OWN_RESULT = offsetof(OwnTables, fault); // what comes down after an encode: fault, bits, vals

// OwnTables' result in host memory
struct OwnResult {
    uint32_t fault, pad;
    uint8_t bits[4][16], vals[4][256];
};
static_assert(sizeof(OwnResult) == offsetof(OwnTables, partial) - OWN_RESULT, "OwnResult is OwnTables from fault to vals");

static int ensure_own(tf_jpeg *enc)
{
    if (enc->own.p)
        return TF_OK;
    TF_TRY(enc->own.alloc(sizeof(OwnTables)));
    TF_TRY(enc->own_tables.alloc(sizeof(Tables)));
    TF_TRY(enc->own_host.alloc(sizeof(OwnResult)));
    TF_HIP(hipMemcpyAsync(enc->own_tables.p, enc->tables.p, sizeof(Tables), hipMemcpyDeviceToDevice, stream()));
    const char *one_lane = getenv("TF_JPEG_TABLES_ONE_LANE");
    enc->one_lane_tables = one_lane && one_lane[0] == '1';
    return TF_OK;
}

static int make_tables(tf_jpeg *enc)
{
    return launch("jpeg_tables", enc->one_lane_tables ? k_jpeg_tables<false> : k_jpeg_tables<true>, dim3(1), dim3(TABLES_BLOCK), 0,
                  enc->own.as<OwnTables>(), enc->own_tables.as<Tables>());
}

static int own_fault(const char *who, uint32_t fault)
{
    for (int t = 0; t < 4; t++)
        if (fault & (1u << t))
            return set_error(TF_ERR_STATE, "%s: the %s table would need a code of more than %d bits (libjpeg's JERR_HUFF_CLEN_OVERFLOW)",
                             who, TABLE_NAMES[t], HUFF_MAX_CLEN);
    for (int t = 0; t < 4; t++)
        if (fault & (16u << t))
            return set_error(TF_ERR_STATE, "%s: the %s table has no symbol", who, TABLE_NAMES[t]);
    return TF_OK;
}

TF_API int tf_jpeg_set_optimize(tf_jpeg *enc, int mode)
{
    TF_REQUIRE(enc, "tf_jpeg_set_optimize: null pointer");
    TF_REQUIRE(mode == 0 || mode == 1, "tf_jpeg_set_optimize: mode %d (0: the Annex K tables, 1: the frame's own)", mode);
    // a frequency stays at or below libjpeg's selection sentinel, and within uint32_t (jpeg_huff.h)
    TF_REQUIRE(mode == 0 || (long long)mcu_blocks(enc->sub) * 64 * enc->n_mcus <= (long long)HUFF_SENTINEL,
               "tf_jpeg_set_optimize: %dx%d has more than %u coefficients", enc->W, enc->H, HUFF_SENTINEL);
    if (mode != enc->optimize) {
        enc->optimize = mode;
        enc->s.last = 0; // the file of the other mode is not this mode's to copy again
        enc->own_header.clear();
    }
    return TF_OK;
}

TF_API void tf_jpeg_destroy(tf_jpeg *enc) { delete enc; }

TF_API int tf_jpeg_create_sub(tf_jpeg **out, int height, int width, int quality, int restart_mcus, int subsampling)
{
    TF_REQUIRE(out, "tf_jpeg_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(height >= 1 && width >= 1 && height <= 65535 && width <= 65535, "tf_jpeg_create: bad size %dx%d (1 to 65535)",
               width, height);
    TF_REQUIRE(quality >= 1 && quality <= 100, "tf_jpeg_create: quality %d (1 to 100)", quality);
    TF_REQUIRE(restart_mcus >= 0 && restart_mcus <= 65535, "tf_jpeg_create: restart interval %d (0 = default, 1 to 65535)",
               restart_mcus);
    if (subsampling != S444 && subsampling != S422 && subsampling != S420)
        return set_error(TF_ERR_UNSUPPORTED, "tf_jpeg_create_sub: subsampling %d (0: 4:4:4, 1: 4:2:2, 2: 4:2:0)", subsampling);
    TF_TRY(ensure_init());
    auto enc = make_handle<tf_jpeg>();
    TF_REQUIRE(enc, "tf_jpeg_create: out of memory");
    enc->H = height, enc->W = width, enc->quality = quality, enc->sub = subsampling;
    enc->restart_mcus = restart_mcus ? restart_mcus : default_restart_mcus(subsampling);
    enc->mcus_x = cdiv(width, mcu_width(subsampling));
    enc->n_mcus = enc->mcus_x * cdiv(height, mcu_height(subsampling)); // (at most 8192 x 8192 = 2^26)
    enc->n_intervals = (enc->n_mcus + enc->restart_mcus - 1) / enc->restart_mcus;

    Tables t;
    uint8_t q[2][64];
    quant_table(QUANT_LUMA, quality, q[0]);
    quant_table(QUANT_CHROMA, quality, q[1]);
    for (int k = 0; k < 64; k++) {
        t.zz[k] = ZIGZAG[k];
        t.q8[0][k] = (uint16_t)(8 * q[0][ZIGZAG[k]]), t.q8[1][k] = (uint16_t)(8 * q[1][ZIGZAG[k]]);
    }
    memcpy(enc->q, q, sizeof(q));
    huff_entries(DC_LUMA_BITS, DC_LUMA_VALS, t.dc[0], 16);
    huff_entries(DC_CHROMA_BITS, DC_CHROMA_VALS, t.dc[1], 16);
    huff_entries(AC_LUMA_BITS, AC_LUMA_VALS, t.ac[0], 256);
    huff_entries(AC_CHROMA_BITS, AC_CHROMA_VALS, t.ac[1], 256);
    enc->header = make_header(height, width, q, enc->restart_mcus, enc->sub);

    for (int c = 0; c < 2; c++) // a lane's symbols: three ZRLs, a code, 10 value bits (11 with a DC code)
        if (3 * (t.ac[c][0xF0] >> 16) + 16 + 10 > (uint32_t)LANE_MAX_BITS)
            return set_error(TF_ERR_STATE, "tf_jpeg_create: a lane's symbols would not fit %d bits", LANE_MAX_BITS);
    TF_TRY(enc->tables.alloc(sizeof(Tables)));
    // (an interval longer than the image codes n_mcus MCUs: its slot need not be larger than that)
    TF_TRY(enc->s.alloc(enc->n_intervals, (uint32_t)slot_bytes(enc->restart_mcus < enc->n_mcus ? enc->restart_mcus : enc->n_mcus, enc->sub), 2));
    TF_HIP(hipMemcpyAsync(enc->tables.p, &t, sizeof(Tables), hipMemcpyHostToDevice, stream()));
    TF_HIP(hipStreamSynchronize(stream())); // `t` is on this stack
    *out = enc.release();
    return TF_OK;
}

TF_API int tf_jpeg_create(tf_jpeg **out, int height, int width, int quality, int restart_mcus)
{
    return tf_jpeg_create_sub(out, height, width, quality, restart_mcus, S420);
}

TF_API int tf_jpeg_header(tf_jpeg *enc, const uint8_t **bytes, size_t *n)
{
    TF_REQUIRE(enc && bytes && n, "tf_jpeg_header: null pointer");
    *bytes = nullptr, *n = 0;
    if (enc->optimize && enc->own_header.empty())
        return set_error(TF_ERR_STATE, "tf_jpeg_header: the header is the frame's, and nothing has been encoded");
    *bytes = enc->file_header().data();
    *n = enc->file_header().size();
    return TF_OK;
}

// one pass of the encode kernel, in the handle's layout
template <int PASS> static int encode_pass(const char *label, const tf_jpeg *enc, const EncodeArgs &a, const FastDiv &div)
{
    const auto kernel = enc->sub == S444   ? k_jpeg_encode<PASS, S444>
                        : enc->sub == S422 ? k_jpeg_encode<PASS, S422>
                                           : k_jpeg_encode<PASS, S420>;
    return launch(label, kernel, dim3(enc->n_intervals), dim3(WAVE), 0, a, div);
}

// the slots to their places in the packed stream, as far as `dev_capacity` reaches
static int pack(tf_jpeg *enc, size_t dev_capacity)
{
    const SlotStream &s = enc->s;
    return launch("jpeg_pack", k_jpeg_pack, dim3(cdiv(s.n, PACK_BLOCK / WAVE)), dim3(PACK_BLOCK), 0, s.staging.as<uint8_t>(), s.slot,
                  s.lengths.as<uint32_t>(), s.offsets.as<uint32_t>(), s.n, s.packed.as<uint8_t>(), dev_capacity);
}

TF_API int tf_jpeg_encode_dev(tf_jpeg *enc, const void *rgb_dev, uint8_t *out, size_t capacity, size_t *n_bytes)
{
    TF_REQUIRE(enc && rgb_dev && n_bytes && (out || capacity == 0), "tf_jpeg_encode_dev: null pointer");
    *n_bytes = 0;
    SlotStream &s = enc->s;
    TF_TRY(s.begin());
    if (enc->optimize) {
        TF_TRY(ensure_own(enc));
        enc->own_header.clear();
        TF_HIP(hipMemsetAsync(enc->own.p, 0, sizeof(OwnTables), stream())); // the histograms and the fault word
    }
    EncodeArgs a;
    a.rgb = (const uint8_t *)rgb_dev, a.W = enc->W, a.H = enc->H;
    a.mcus_x = enc->mcus_x, a.n_mcus = enc->n_mcus, a.restart_mcus = enc->restart_mcus;
    a.lum_bx = (enc->W + 7) / 8, a.lum_by = (enc->H + 7) / 8, a.chroma_rows = (enc->H + 1) / 2;
    a.tables = enc->tables.as<Tables>(), a.staging = s.staging.as<uint8_t>(), a.slot_bytes = s.slot;
    a.lengths = s.lengths.as<uint32_t>();
    a.overflow = s.overflow();
    a.counts = nullptr;
    const FastDiv div = fast_div_setup((uint32_t)enc->mcus_x);
    if (enc->optimize) { // count, make the tables, code with them
        OwnTables *own = enc->own.as<OwnTables>();
        a.counts = &own->partial[0][0][0];
        TF_TRY(encode_pass<GATHER>("jpeg_gather", enc, a, div));
        TF_TRY(make_tables(enc));
        a.tables = enc->own_tables.as<Tables>();
        TF_TRY(encode_pass<EMIT_WIDE>("jpeg_emit", enc, a, div));
    } else {
        TF_TRY(encode_pass<EMIT>("jpeg_encode", enc, a, div));
    }
    TF_TRY(s.scan("jpeg_scan"));
    // (the frame's own header is not known before the kernels have run)
    TF_TRY(pack(enc, enc->optimize ? s.pack_room() : s.pack_room(capacity, enc->header.size())));
    TF_TRY(s.fetch());
    if (enc->optimize) // comes down with the stream's info: the one wait below is for both
        TF_HIP(hipMemcpyAsync(enc->own_host.p, (const uint8_t *)enc->own.p + OWN_RESULT, sizeof(OwnResult), hipMemcpyDeviceToHost,
                              stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    if (enc->optimize) {
        const OwnResult &r = *enc->own_host.as<OwnResult>();
        TF_TRY(own_fault("tf_jpeg_encode_dev", r.fault));
        const Dht dht[4] = {{r.bits[0], r.vals[0]}, {r.bits[1], r.vals[1]}, {r.bits[2], r.vals[2]}, {r.bits[3], r.vals[3]}};
        enc->own_header = make_header(enc->H, enc->W, enc->q, enc->restart_mcus, enc->sub, dht);
    }
    TF_TRY(s.finish("tf_jpeg_encode_dev", "an interval"));
    return s.copy_out("tf_jpeg_encode_dev", enc->file_header(), {}, out, capacity, n_bytes);
}

TF_API int tf_jpeg_copy_last(tf_jpeg *enc, uint8_t *out, size_t capacity, size_t *n_bytes)
{
    TF_REQUIRE(enc && n_bytes && (out || capacity == 0), "tf_jpeg_copy_last: null pointer");
    *n_bytes = 0;
    TF_TRY(enc->s.have_last("tf_jpeg_copy_last"));
    TF_TRY(pack(enc, enc->s.pack_room(capacity, enc->file_header().size())));
    return enc->s.copy_out("tf_jpeg_copy_last", enc->file_header(), {}, out, capacity, n_bytes);
}

TF_API int tf_jpeg_last_tables(tf_jpeg *enc, uint8_t *bits, uint8_t *vals, uint32_t *counts)
{
    TF_REQUIRE(enc && bits && vals, "tf_jpeg_last_tables: null pointer");
    if (!enc->optimize || enc->own_header.empty())
        return set_error(TF_ERR_STATE, "tf_jpeg_last_tables: no encode with the frame's own tables has run");
    const OwnResult &r = *enc->own_host.as<OwnResult>();
    memcpy(bits, r.bits, sizeof(r.bits));
    memcpy(vals, r.vals, sizeof(r.vals));
    if (counts) {
        TF_HIP(hipMemcpyAsync(counts, enc->own.p, sizeof(uint32_t) * 4 * 257, hipMemcpyDeviceToHost, stream()));
        TF_HIP(hipStreamSynchronize(stream()));
        for (int t = 0; t < 4; t++)
            counts[t * 257 + 256] = 1; // the reserved symbol: the gather pass does not count it
    }
    return TF_OK;
}

TF_API int tf_jpeg_tables_from_counts(tf_jpeg *enc, const uint32_t *counts, uint8_t *bits, uint8_t *vals, uint32_t *fault)
{
    TF_REQUIRE(enc && counts && bits && vals && fault, "tf_jpeg_tables_from_counts: null pointer");
    *fault = 0;
    for (int t = 0; t < 4; t++) {
        unsigned long long sum = 0;
        for (int i = 0; i < 256; i++)
            sum += counts[t * 257 + i];
        TF_REQUIRE(sum > 0, "tf_jpeg_tables_from_counts: the %s histogram has no symbol", TABLE_NAMES[t]);
        TF_REQUIRE(sum <= HUFF_SENTINEL, "tf_jpeg_tables_from_counts: the %s histogram sums to more than %u", TABLE_NAMES[t],
                   HUFF_SENTINEL);
    }
    TF_TRY(ensure_own(enc));
    enc->own_header.clear(), enc->s.last = 0; // the tables of the last encode are gone
    OwnTables *own = enc->own.as<OwnTables>();
    TF_HIP(hipMemsetAsync(enc->own.p, 0, sizeof(OwnTables), stream()));
    TF_HIP(hipMemcpyAsync(own->partial[0], counts, sizeof(own->counts), hipMemcpyHostToDevice, stream())); // the other copies are zero
    TF_TRY(make_tables(enc));
    TF_HIP(hipMemcpyAsync(enc->own_host.p, (const uint8_t *)enc->own.p + OWN_RESULT, sizeof(OwnResult), hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    const OwnResult &r = *enc->own_host.as<OwnResult>();
    *fault = r.fault;
    memcpy(bits, r.bits, sizeof(r.bits));
    memcpy(vals, r.vals, sizeof(r.vals));
    return own_fault("tf_jpeg_tables_from_counts", r.fault);
}

TF_API int tf_jpeg_default_restart_mcus(void) { return DEFAULT_RESTART_MCUS; }

TF_API int tf_jpeg_default_restart_mcus_for(int subsampling)
{
    if (subsampling != S444 && subsampling != S422 && subsampling != S420)
        return set_error(TF_ERR_UNSUPPORTED, "tf_jpeg_default_restart_mcus_for: subsampling %d (0: 4:4:4, 1: 4:2:2, 2: 4:2:0)",
                         subsampling);
    return default_restart_mcus(subsampling);
}

TF_API int tf_jpeg_encode(tf_jpeg *enc, const uint8_t *rgb_host, uint8_t *out, size_t capacity, size_t *n_bytes)
{
    TF_REQUIRE(enc && rgb_host && n_bytes, "tf_jpeg_encode: null pointer");
    const size_t bytes = (size_t)enc->H * enc->W * 3;
    TF_TRY(enc->upload.upload(rgb_host, bytes));
    return tf_jpeg_encode_dev(enc, enc->upload.p, out, capacity, n_bytes);
}
