// Baseline JPEG decoded on the device (jpegdec.hip): the part of the decoder that decides what is in bounds -- the
// segment walker, the table builder, the bit reader, the per-block step -- and the arithmetic that is pinned to libjpeg
// (jidctint.c's islow IDCT), as host/device inline functions over plain memory.  The kernels run them over LDS;
// tools/jpegdec_host_check.cpp runs the same functions on the CPU under the sanitizers (DESIGN.md section 19;
// tests/jpegdec_ref.py is the Python statement of the same rules).
//
// A file is taken whole or rejected whole (Reject).  The header is walked on the host; what lies behind SOS is only
// looked at on the device: FF D0..D7 pairs separate the restart intervals (inside entropy-coded data an FF is always
// followed by 00), and every interval is decoded on its own from a byte range nothing else owns.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JD_HD __host__ __device__ inline
#else
#define JD_HD inline
#endif

namespace tf {
namespace jpegdec {

// why a file was rejected (0: it was not); the names are tests/jpegdec_ref.py's.  Where a file has several faults the
// first stage that sees one reports: the header, then the marker scan (the lowest number), then the lowest interval.
enum Reject : uint32_t {
    R_OK = 0,
    R_NOT_JPEG = 1,         // no SOI
    R_TRUNCATED = 2,        // the file ends before SOS is complete
    R_BAD_SEGMENT = 3,      // a segment's length or content is malformed, a marker that has no place before SOS
    R_PROGRESSIVE = 4,      // SOF2
    R_ARITHMETIC = 5,       // SOF9 .. SOF15, DAC
    R_SOF_KIND = 6,         // any other SOF but SOF0 (extended, lossless, differential)
    R_PRECISION = 7,        // samples that are not 8-bit
    R_COMPONENTS = 8,       // neither 1 nor 3 components
    R_SAMPLING = 9,         // luma not 2x2, 2x1 or 1x1, chroma not 1x1
    R_MULTI_SCAN = 10,      // the scan does not interleave all components over the whole spectrum
    R_DNL = 11,             // a height of 0 (to be given by DNL)
    R_ADOBE_TRANSFORM = 12, // an Adobe APP14 segment with transform 0 or 2
    R_DQT_16BIT = 13,
    R_MISSING_TABLE = 14,   // a table the scan names and the file lacks
    R_BAD_DHT = 15,         // an over-subscribed or malformed Huffman table
    R_NO_EOI = 16,          // the file does not end with EOI
    R_STRAY_MARKER = 17,    // a marker inside the scan that is no RSTn
    R_RST_COUNT = 18,       // a restart marker missing, or one too many (any at all where DRI gives none)
    R_RST_ORDER = 19,       // marker k is not RST(k mod 8)
    R_BAD_CODE = 20,        // bits that match no code
    R_BAD_SYMBOL = 21,      // an AC symbol with size 0 and a run that is neither 0 (EOB) nor 15 (ZRL)
    R_RUN_PAST_63 = 22,     // a run that passes coefficient 63
    R_CATEGORY = 23,        // a magnitude category above 11 (DC) or 10 (AC)
    R_DC_RANGE = 24,        // a DC value outside +-2047
    R_EXHAUSTED = 25,       // the interval's bytes run out inside an MCU
    R_COUNT = 26,
};

JD_HD const char *reject_name(uint32_t r)
{
    switch (r) {
    case R_OK: return "ok";
    case R_NOT_JPEG: return "not_jpeg";
    case R_TRUNCATED: return "truncated";
    case R_BAD_SEGMENT: return "bad_segment";
    case R_PROGRESSIVE: return "progressive";
    case R_ARITHMETIC: return "arithmetic";
    case R_SOF_KIND: return "sof_kind";
    case R_PRECISION: return "precision";
    case R_COMPONENTS: return "components";
    case R_SAMPLING: return "sampling";
    case R_MULTI_SCAN: return "multi_scan";
    case R_DNL: return "dnl";
    case R_ADOBE_TRANSFORM: return "adobe_transform";
    case R_DQT_16BIT: return "dqt_16bit";
    case R_MISSING_TABLE: return "missing_table";
    case R_BAD_DHT: return "bad_dht";
    case R_NO_EOI: return "no_eoi";
    case R_STRAY_MARKER: return "stray_marker";
    case R_RST_COUNT: return "rst_count";
    case R_RST_ORDER: return "rst_order";
    case R_BAD_CODE: return "bad_code";
    case R_BAD_SYMBOL: return "bad_symbol";
    case R_RUN_PAST_63: return "run_past_63";
    case R_CATEGORY: return "category";
    case R_DC_RANGE: return "dc_range";
    case R_EXHAUSTED: return "exhausted";
    default: return "unknown";
    }
}

constexpr int FAST_BITS = 9;
constexpr uint32_t WINDOW_BYTES = 1024; // bytes of the interval in reach of the bit reader
// A block is at most 64 symbols (every AC symbol advances the coefficient index) of a 16-bit code and at most 11 value
// bits (a larger category is rejected before its bits are taken): 1728 bits, 216 bytes, each of which may be an FF with
// its 00; the reader runs at most 8 bytes ahead.
constexpr uint32_t BLOCK_MARGIN = 2 * 216 + 16;
static_assert(BLOCK_MARGIN <= WINDOW_BYTES, "a block must fit the window");
constexpr int MAX_BLOCKS = 6; // blocks per MCU: 4:2:0

constexpr uint8_t ZIGZAG[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};

// ---- a Huffman table as the decoder reads it (jdhuff.c jpeg_make_d_derived_tbl) --------------------------------------
struct Huff {
    int32_t maxcode[17];         // the largest code of each length, -1 where there is none
    int32_t valoff[17];          // vals index of a length's first code minus that code
    uint16_t fast[1 << FAST_BITS]; // by the next FAST_BITS bits: (length << 8) | symbol, 0 where no such code starts
    uint8_t vals[256];
};
static_assert(sizeof(Huff) % 4 == 0, "tables are copied by dwords");

// counts[16], then `n_vals` symbols.  false: more than 256 symbols, more than the segment holds, a code that does not
// fit its length or is all ones (libjpeg's rule), a DC symbol above 15.
JD_HD bool build_huff(Huff &h, const uint8_t *counts, const uint8_t *vals, size_t n_vals, bool is_dc)
{
    uint32_t total = 0;
    for (int l = 0; l < 16; l++)
        total += counts[l];
    if (total > 256 || total > n_vals)
        return false;
    for (int i = 0; i < (1 << FAST_BITS); i++)
        h.fast[i] = 0;
    for (int i = 0; i < 256; i++)
        h.vals[i] = 0;
    for (uint32_t i = 0; i < total; i++) {
        if (is_dc && vals[i] > 15)
            return false;
        h.vals[i] = vals[i];
    }
    uint32_t code = 0, p = 0;
    h.maxcode[0] = -1, h.valoff[0] = 0;
    for (int l = 1; l <= 16; l++) {
        const uint32_t n = counts[l - 1];
        h.valoff[l] = (int32_t)p - (int32_t)code;
        h.maxcode[l] = n ? (int32_t)(code + n - 1) : -1;
        if (n && code + n >= (1u << l))
            return false;
        if (l <= FAST_BITS)
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t first = (code + k) << (FAST_BITS - l);
                for (uint32_t j = 0; j < (1u << (FAST_BITS - l)); j++)
                    h.fast[first + j] = (uint16_t)(((uint32_t)l << 8) | vals[p + k]); // (first + j < 2^FAST_BITS: code + k < 2^l)
            }
        p += n;
        code = (code + n) << 1;
    }
    return true;
}

// ---- the header ----------------------------------------------------------------------------------------------------
struct Header {
    int width, height, components, h_samp, v_samp, restart_mcus;
    int mcus_x, mcus_y, n_mcus, intervals, blocks_per_mcu;
    size_t scan_offset;      // the first byte behind SOS
    uint16_t quant[3][64];   // per component, by zigzag position
    Huff dc[3], ac[3];       // per component
};

struct Raw { // what the segments gave, until SOS says which of it is used
    uint8_t have_q[4], have_dc[4], have_ac[4];
    uint16_t q[4][64];
    Huff dc[4], ac[4];
};

JD_HD uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }

// Walks file[0, n) up to and including SOS.  `raw` is working space.  Every index is checked against n first.
JD_HD uint32_t parse_header(const uint8_t *file, size_t n, Header &hd, Raw &raw)
{
    if (n < 2)
        return n == 0 || file[0] == 0xFF ? R_TRUNCATED : R_NOT_JPEG;
    if (file[0] != 0xFF || file[1] != 0xD8)
        return R_NOT_JPEG;
    for (int i = 0; i < 4; i++)
        raw.have_q[i] = raw.have_dc[i] = raw.have_ac[i] = 0;
    bool have_sof = false;
    uint8_t comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
    hd.restart_mcus = 0;
    size_t at = 2;
    for (;;) {
        if (n - at < 2)
            return R_TRUNCATED;
        if (file[at] != 0xFF)
            return R_BAD_SEGMENT;
        const uint32_t marker = file[at + 1];
        if (marker == 0xFF) { // a fill byte
            at++;
            continue;
        }
        at += 2;
        if (marker == 0xD9)
            return R_TRUNCATED; // EOI before any scan
        if (marker == 0xD8 || marker == 0x01 || marker == 0x00 || (marker >= 0xD0 && marker <= 0xD7))
            return R_BAD_SEGMENT;
        if (n - at < 2)
            return R_TRUNCATED;
        const size_t len = be16(file + at);
        if (len < 2)
            return R_BAD_SEGMENT;
        if (n - at < len)
            return R_TRUNCATED;
        const uint8_t *p = file + at + 2;
        const size_t m = len - 2; // the payload: p[0, m)
        at += len;
        if (marker == 0xC0 || marker == 0xC1 || marker == 0xC2 || marker == 0xC3 || (marker >= 0xC5 && marker <= 0xC7) ||
            (marker >= 0xC9 && marker <= 0xCB) || (marker >= 0xCD && marker <= 0xCF)) {
            if (marker == 0xC2)
                return R_PROGRESSIVE;
            if (marker >= 0xC9)
                return R_ARITHMETIC;
            if (marker != 0xC0)
                return R_SOF_KIND;
            if (have_sof || m < 6)
                return R_BAD_SEGMENT;
            if (p[0] != 8)
                return R_PRECISION;
            hd.height = (int)be16(p + 1), hd.width = (int)be16(p + 3), hd.components = p[5];
            if (hd.components != 1 && hd.components != 3)
                return R_COMPONENTS;
            if (m != 6 + 3 * (size_t)hd.components)
                return R_BAD_SEGMENT;
            if (hd.height == 0)
                return R_DNL;
            if (hd.width == 0)
                return R_BAD_SEGMENT;
            for (int c = 0; c < hd.components; c++) {
                comp_id[c] = p[6 + 3 * c];
                const int hs = p[7 + 3 * c] >> 4, vs = p[7 + 3 * c] & 15;
                comp_tq[c] = p[8 + 3 * c];
                if (comp_tq[c] > 3)
                    return R_BAD_SEGMENT;
                if (c == 0) {
                    hd.h_samp = hs, hd.v_samp = vs;
                    const bool ok = hd.components == 1 ? (hs == 1 && vs == 1) : ((hs == 2 && (vs == 2 || vs == 1)) || (hs == 1 && vs == 1));
                    if (!ok)
                        return R_SAMPLING;
                } else if (hs != 1 || vs != 1) {
                    return R_SAMPLING;
                }
            }
            have_sof = true;
        } else if (marker == 0xCC) {
            return R_ARITHMETIC;
        } else if (marker == 0xC4) {
            size_t k = 0;
            while (k < m) {
                if (m - k < 17)
                    return R_BAD_DHT;
                const uint32_t tc = p[k] >> 4, th = p[k] & 15;
                if (tc > 1 || th > 3)
                    return R_BAD_DHT;
                uint32_t total = 0;
                for (int l = 0; l < 16; l++)
                    total += p[k + 1 + l];
                Huff &h = tc ? raw.ac[th] : raw.dc[th];
                if (!build_huff(h, p + k + 1, p + k + 17, m - k - 17, tc == 0))
                    return R_BAD_DHT;
                (tc ? raw.have_ac : raw.have_dc)[th] = 1;
                k += 17 + total;
            }
        } else if (marker == 0xDB) {
            size_t k = 0;
            while (k < m) {
                const uint32_t pq = p[k] >> 4, tq = p[k] & 15;
                if (pq == 1)
                    return R_DQT_16BIT;
                if (pq > 1 || tq > 3 || m - k < 65)
                    return R_BAD_SEGMENT;
                for (int i = 0; i < 64; i++)
                    raw.q[tq][i] = p[k + 1 + i];
                raw.have_q[tq] = 1;
                k += 65;
            }
        } else if (marker == 0xDD) {
            if (m != 2)
                return R_BAD_SEGMENT;
            hd.restart_mcus = (int)be16(p);
        } else if (marker == 0xDC) {
            return R_DNL;
        } else if (marker == 0xEE) {
            if (m >= 12 && p[0] == 'A' && p[1] == 'd' && p[2] == 'o' && p[3] == 'b' && p[4] == 'e' && p[11] != 1)
                return R_ADOBE_TRANSFORM;
        } else if (marker == 0xDA) {
            if (!have_sof || m < 1)
                return R_BAD_SEGMENT;
            const int ns = p[0];
            if (ns != hd.components)
                return R_MULTI_SCAN;
            if (m != 4 + 2 * (size_t)ns)
                return R_BAD_SEGMENT;
            for (int c = 0; c < ns; c++) {
                if (p[1 + 2 * c] != comp_id[c])
                    return R_MULTI_SCAN;
                const uint32_t td = p[2 + 2 * c] >> 4, ta = p[2 + 2 * c] & 15;
                if (td > 3 || ta > 3)
                    return R_BAD_SEGMENT;
                if (!raw.have_dc[td] || !raw.have_ac[ta] || !raw.have_q[comp_tq[c]])
                    return R_MISSING_TABLE;
                hd.dc[c] = raw.dc[td], hd.ac[c] = raw.ac[ta];
                for (int i = 0; i < 64; i++)
                    hd.quant[c][i] = raw.q[comp_tq[c]][i];
            }
            if (p[1 + 2 * ns] != 0 || p[2 + 2 * ns] != 63 || p[3 + 2 * ns] != 0)
                return R_MULTI_SCAN;
            hd.scan_offset = at;
            const int mw = 8 * hd.h_samp, mh = 8 * hd.v_samp;
            hd.mcus_x = (hd.width + mw - 1) / mw, hd.mcus_y = (hd.height + mh - 1) / mh; // at most 8192 each
            hd.n_mcus = hd.mcus_x * hd.mcus_y;
            hd.blocks_per_mcu = hd.components == 1 ? 1 : hd.h_samp * hd.v_samp + 2;
            hd.intervals = hd.restart_mcus ? (hd.n_mcus + hd.restart_mcus - 1) / hd.restart_mcus : 1;
            return R_OK;
        } else if ((marker >= 0xE0 && marker <= 0xEF) || marker == 0xFE) {
            // APPn, COM: skipped
        } else {
            return R_BAD_SEGMENT;
        }
    }
}

// ---- the marker scan: what the byte behind an FF of the scan makes of the pair ------------------------------------------
enum PairKind : uint32_t { P_STUFFED = 0, P_RST = 1, P_STRAY = 2 };
JD_HD uint32_t pair_kind(uint8_t behind) { return behind == 0 ? P_STUFFED : (behind >= 0xD0 && behind <= 0xD7 ? P_RST : P_STRAY); }

// ---- the bit reader: bytes [0, size) of the interval, of which win[0 .. win_len) holds those from win_base on ---------
struct Bits {
    const uint8_t *win;
    uint32_t win_base, win_len;
    uint32_t size; // the interval's bytes
    uint32_t next; // the next byte of the interval to take into buf
    uint64_t buf;  // cnt bits, the stream's next bit the highest of them
    uint32_t cnt;
};

JD_HD void start(Bits &b, const uint8_t *win, uint32_t size)
{
    b.win = win, b.win_base = 0, b.win_len = 0, b.size = size, b.next = 0, b.buf = 0, b.cnt = 0;
}

// whether `margin` bytes from the reader's place on are in the window (or the window reaches the interval's end)
JD_HD bool need_refill(const Bits &b, uint32_t margin)
{
    const uint64_t have = (uint64_t)b.win_base + b.win_len;
    return have < b.size && (uint64_t)b.next + margin > have;
}

// the window becomes bytes [*from, *from + *len) of the interval
JD_HD void refill_range(Bits &b, uint32_t *from, uint32_t *len)
{
    b.win_base = b.next; // (next <= size)
    b.win_len = b.size - b.next < WINDOW_BYTES ? b.size - b.next : WINDOW_BYTES;
    *from = b.win_base, *len = b.win_len;
}

// more than 56 bits in buf afterwards, or every bit the window has left; FF 00 gives FF, an FF before anything else
// (there is none in an interval the marker scan passed) or at the very end ends the data
JD_HD void fill(Bits &b)
{
    while (b.cnt <= 56 && b.next < b.size) {
        const uint32_t k = b.next - b.win_base; // (next >= win_base: the window only moves to `next`)
        if (k >= b.win_len)
            break;
        const uint32_t v = b.win[k];
        if (v == 0xFF) {
            if (k + 1 >= b.win_len || b.win[k + 1] != 0)
                break;
            b.next++;
        }
        b.buf = (b.buf << 8) | v;
        b.cnt += 8;
        b.next++;
    }
}

JD_HD uint32_t peek16(const Bits &b) // the next 16 bits, zeros behind the last
{
    return (uint32_t)(b.cnt >= 16 ? b.buf >> (b.cnt - 16) : b.buf << (16 - b.cnt)) & 0xFFFFu;
}

// n <= 16 bits, or false: the interval has fewer left
JD_HD bool take(Bits &b, uint32_t n, uint32_t &v)
{
    if (b.cnt < n)
        fill(b);
    if (b.cnt < n)
        return false;
    v = (uint32_t)(b.buf >> (b.cnt - n)) & ((1u << n) - 1);
    b.cnt -= n;
    return true;
}

// the next symbol: R_OK, R_EXHAUSTED (the interval ends inside the code) or R_BAD_CODE (16 bits that are no code)
JD_HD uint32_t decode(Bits &b, const Huff &h, uint32_t &sym)
{
    if (b.cnt < 16)
        fill(b);
    const uint32_t bits = peek16(b);
    const uint32_t e = h.fast[bits >> (16 - FAST_BITS)];
    if (e) {
        const uint32_t len = e >> 8;
        if (len > b.cnt)
            return R_EXHAUSTED;
        b.cnt -= len;
        sym = e & 255u;
        return R_OK;
    }
    for (int len = FAST_BITS + 1; len <= 16; len++) {
        const int32_t code = (int32_t)(bits >> (16 - len));
        if (code <= h.maxcode[len]) {
            if ((uint32_t)len > b.cnt)
                return R_EXHAUSTED;
            const int32_t at = h.valoff[len] + code;
            if (at < 0 || at > 255)
                return R_BAD_CODE; // (never: build_huff counted at most 256 symbols)
            b.cnt -= (uint32_t)len;
            sym = h.vals[at];
            return R_OK;
        }
    }
    return b.cnt < 16 ? R_EXHAUSTED : R_BAD_CODE;
}

JD_HD int extend(uint32_t v, uint32_t s) { return v < (1u << (s - 1)) ? (int)v - (int)(1u << s) + 1 : (int)v; } // HUFF_EXTEND, 1 <= s <= 11

// One block (jdhuff.c decode_mcu): coef[64], zero on entry, gets the dequantised coefficients in natural order.
// last_dc: the component's prediction, 0 at the start of an interval.
JD_HD uint32_t decode_block(Bits &b, const Huff &dc, const Huff &ac, const uint16_t *quant, int &last_dc, int32_t *coef)
{
    uint32_t s, v;
    uint32_t rc = decode(b, dc, s);
    if (rc != R_OK)
        return rc;
    if (s > 11)
        return R_CATEGORY;
    int diff = 0;
    if (s) {
        if (!take(b, s, v))
            return R_EXHAUSTED;
        diff = extend(v, s);
    }
    last_dc += diff; // both within +-2047
    if (last_dc < -2047 || last_dc > 2047)
        return R_DC_RANGE;
    coef[0] = last_dc * (int32_t)quant[0];
    for (uint32_t k = 1; k < 64; k++) {
        rc = decode(b, ac, s);
        if (rc != R_OK)
            return rc;
        const uint32_t r = s >> 4;
        s &= 15;
        if (s) {
            k += r;
            if (k > 63)
                return R_RUN_PAST_63;
            if (s > 10)
                return R_CATEGORY;
            if (!take(b, s, v))
                return R_EXHAUSTED;
            coef[ZIGZAG[k]] = extend(v, s) * (int32_t)quant[k];
        } else if (r == 15) {
            k += 15;
            if (k > 63)
                return R_RUN_PAST_63;
        } else if (r == 0) {
            break;
        } else {
            return R_BAD_SYMBOL;
        }
    }
    return R_OK;
}

// ---- jidctint.c jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2): one pass over 8 values `stride` apart.  The products
// and sums are taken modulo 2^32 (a file's coefficients can be large enough to pass 31 bits; what such a file decodes
// to is not pinned) and shifted as two's complement numbers, which is libjpeg's arithmetic wherever that is defined.
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
JD_HD uint32_t mulc(int32_t a, int32_t c) { return (uint32_t)a * (uint32_t)c; }
JD_HD int32_t descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; } // an arithmetic shift

JD_HD void idct_pass(const int32_t *in, int stride, int shift, int32_t *out /*8*/)
{
    const int32_t i0 = in[0], i1 = in[stride], i2 = in[2 * stride], i3 = in[3 * stride];
    const int32_t i4 = in[4 * stride], i5 = in[5 * stride], i6 = in[6 * stride], i7 = in[7 * stride];
    uint32_t z1 = mulc((int32_t)((uint32_t)i2 + (uint32_t)i6), 4433);                // FIX_0_541196100
    const uint32_t t2 = z1 + mulc(i6, -15137), t3 = z1 + mulc(i2, 6270);            // FIX_1_847759065, FIX_0_765366865
    const uint32_t t0 = ((uint32_t)i0 + (uint32_t)i4) << CONST_BITS, t1 = ((uint32_t)i0 - (uint32_t)i4) << CONST_BITS;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int32_t s1 = (int32_t)((uint32_t)i7 + (uint32_t)i1), s2 = (int32_t)((uint32_t)i5 + (uint32_t)i3);
    const int32_t s3 = (int32_t)((uint32_t)i7 + (uint32_t)i3), s4 = (int32_t)((uint32_t)i5 + (uint32_t)i1);
    const uint32_t z5 = mulc((int32_t)((uint32_t)s3 + (uint32_t)s4), 9633);          // FIX_1_175875602
    uint32_t o0 = mulc(i7, 2446), o1 = mulc(i5, 16819), o2 = mulc(i3, 25172), o3 = mulc(i1, 12299);
    z1 = mulc(s1, -7373);                                                            // FIX_0_899976223
    const uint32_t z2 = mulc(s2, -20995);                                            // FIX_2_562915447
    const uint32_t z3 = mulc(s3, -16069) + z5, z4 = mulc(s4, -3196) + z5;           // FIX_1_961570560, FIX_0_390180644
    o0 += z1 + z3, o1 += z2 + z4, o2 += z2 + z3, o3 += z1 + z4;
    out[0] = descale(t10 + o3, shift), out[7] = descale(t10 - o3, shift);
    out[1] = descale(t11 + o2, shift), out[6] = descale(t11 - o2, shift);
    out[2] = descale(t12 + o1, shift), out[5] = descale(t12 - o1, shift);
    out[3] = descale(t13 + o0, shift), out[4] = descale(t13 - o0, shift);
}

// the sample of a row-pass result: range_limit[x & RANGE_MASK] of the table centred on 128
JD_HD uint8_t range_limit(int32_t x)
{
    const uint32_t i = (uint32_t)x & 1023u;
    return (uint8_t)(i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896)));
}

// a block: coef[64] (natural order) -> ws[64] by columns, then row `r` of ws -> 8 samples
JD_HD void idct_column(const int32_t *coef, int col, int32_t *ws)
{
    int32_t o[8];
    idct_pass(coef + col, 8, CONST_BITS - PASS1_BITS, o);
    for (int i = 0; i < 8; i++)
        ws[8 * i + col] = o[i];
}
JD_HD void idct_row(const int32_t *ws, int row, uint8_t *samples /*8*/)
{
    int32_t o[8];
    idct_pass(ws + 8 * row, 1, CONST_BITS + PASS1_BITS + 3, o);
    for (int i = 0; i < 8; i++)
        samples[i] = range_limit(o[i]);
}

} // namespace jpegdec
} // namespace tf
