// A scan without restart markers decoded side by side (jpegdec.hip's second entropy path; DESIGN.md section 19,
// "scans without restart markers"): the grid of subsequences, the bit window, and the one lane function that both the
// synchronisation phase (lenient, nothing stored) and the write phase (strict, coefficients stored) run, as host/device
// inline functions.  tools/jpegdec_par_host_check.cpp runs them on the CPU under the sanitizers; tests/jpegdec_par_ref.py
// is the Python statement of the same rules.
//
// The scan minus its EOI is `size` bytes; subsequence i is bytes [i * S, (i + 1) * S) of it, stuffed bytes included.  A
// position is a bit index into those bytes and never lies inside the 00 of an FF 00 pair (a position that would is the
// first bit behind the pair).  A decoder's state is (position, block within the MCU, coefficient index k; k = 0: a DC
// code comes next), packed into one word.  A symbol and its value bits are taken together, and a lane stops at the first
// symbol boundary at or behind its subsequence's end.
//
// The lenient rules (synchronisation phase; no fault ends a chain there):
//   16 bits that match no code       skip one bit
//   a run past coefficient 63        the symbol is consumed, its value bits are not; the block ends
//   an AC symbol that is no symbol   the block ends
//   a category above 11 (DC), 10 (AC) the value bits of the largest legal category are taken instead
//   fewer bits left than a symbol or its value needs: the lane ends at the end of the data, (block, k) as they were
// The strict phase gives decode_block's verdicts, in decode_block's order, and stops at the first.
#pragma once
#include "jpegdec_common.h"

namespace tf {
namespace jpegdec {

constexpr int PAR_REASON_BITS = 5; // a strict fault: (subsequence << PAR_REASON_BITS) | reason; the lowest wins
static_assert(R_COUNT <= (1 << PAR_REASON_BITS), "a reason must fit its bits");
constexpr uint32_t PAR_NO_FAULT = 0xFFFFFFFFu;
constexpr uint32_t PAR_MIN_SUB = 16, PAR_MAX_SUB = 1024; // bytes of a subsequence

// (position << 9) | (block << 6) | k: positions are below 2^33 (a scan of at most 2^30 bytes)
JD_HD uint64_t par_pack(uint64_t pos, uint32_t blk, uint32_t k) { return (pos << 9) | ((uint64_t)blk << 6) | k; }
JD_HD uint64_t par_pos(uint64_t s) { return s >> 9; }
JD_HD uint32_t par_blk(uint64_t s) { return (uint32_t)(s >> 6) & 7u; }
JD_HD uint32_t par_k(uint64_t s) { return (uint32_t)s & 63u; }

struct ParGeom {
    uint32_t size;         // the scan's bytes without the EOI
    uint32_t sub_bytes;    // S
    uint32_t n_subs;       // max(1, ceil(size / S))
    uint32_t blocks, luma_blocks; // per MCU
    uint32_t total_blocks; // n_mcus * blocks: what the coefficient buffer holds
};

JD_HD uint32_t par_subs(uint32_t size, uint32_t sub_bytes) { return size ? (size + sub_bytes - 1) / sub_bytes : 1u; }

// ---- the bit window: the 8 bytes from a position's byte on (zeros behind the data), their stuffed zeros removed ---------
struct ParWin {
    uint64_t bits;    // the data bytes, the first one highest; at least 4 of them (32 bits), zeros behind
    uint32_t stuffed; // bit t: byte t of the 8 is the 00 of an FF 00 pair (never byte 0: a position is not inside a pair)
    uint64_t base;    // the byte index of byte 0
};

JD_HD uint32_t par_popc(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}

// where a lane's bytes come from: at(i), i < size, is byte i of the scan.  ParBytes is the scan as it lies in memory;
// jpegdec.hip has a second source that reads a work-group's share from LDS.
struct ParBytes {
    const uint8_t *scan;
    JD_HD uint32_t at(uint64_t i) const { return scan[i]; }
};

template <typename Src> JD_HD ParWin par_window(const Src &src, uint32_t size, uint64_t pos)
{
    ParWin w;
    w.base = pos >> 3;
    uint64_t x = 0;
    uint32_t stuffed = 0, prev = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8; t++) {
        const uint32_t v = w.base + t < size ? src.at(w.base + t) : 0u; // every index is checked against the data's size
        x = (x << 8) | v;
        if (t && prev == 0xFF && v == 0)
            stuffed |= 1u << t;
        prev = v;
    }
#pragma unroll
    for (int t = 7; t >= 1; t--)
        if (stuffed & (1u << t)) {
            const uint64_t low = ((uint64_t)1 << (8 * (7 - t))) - 1; // the bytes behind byte t
            x = (x & ~((low << 8) | 0xFFu)) | ((x & low) << 8);
        }
    w.bits = x, w.stuffed = stuffed;
    return w;
}

// n <= 16 bits from bit `o` of the window on; o + n <= 32
JD_HD uint32_t par_peek(const ParWin &w, uint32_t o, uint32_t n) { return (uint32_t)(w.bits >> (64 - o - n)) & ((1u << n) - 1u); }

// the position n bits behind `pos` (the window's own), (pos & 7) + n < 32: the data byte it falls into is in the window
JD_HD uint64_t par_advance(const ParWin &w, uint64_t pos, uint32_t n)
{
    const uint32_t bit = (uint32_t)(pos & 7) + n, j = bit >> 3; // data byte j <= 3
    uint32_t u = j;
#pragma unroll
    for (int it = 0; it < 4; it++) // the least u with u - (stuffed bytes among 0 .. u) = j: at most 4 stuffed bytes in 8
        u = j + par_popc(w.stuffed & ((2u << u) - 1u));
    return (w.base + u) * 8 + (bit & 7);
}

// the code the 16 bits begin with: its length and symbol, or false
JD_HD bool par_lookup(const Huff &h, uint32_t bits, uint32_t &len, uint32_t &sym)
{
    const uint32_t e = h.fast[bits >> (16 - FAST_BITS)];
    if (e) {
        len = e >> 8, sym = e & 255u;
        return true;
    }
    for (int l = FAST_BITS + 1; l <= 16; l++) {
        const int32_t code = (int32_t)(bits >> (16 - l));
        if (code <= h.maxcode[l]) {
            const int32_t at = h.valoff[l] + code;
            if (at < 0 || at > 255)
                return false; // (never: build_huff counted at most 256 symbols)
            len = (uint32_t)l, sym = h.vals[at];
            return true;
        }
    }
    return false;
}

// the first guess of subsequence i's entry: its first bit, a DC code of the MCU's first block
JD_HD uint64_t par_guess(const uint8_t *scan, uint32_t size, uint32_t sub_bytes, uint32_t i)
{
    uint64_t at = (uint64_t)i * sub_bytes;
    if (i && at < size && scan[at] == 0 && scan[at - 1] == 0xFF) // (at - 1 < size: at >= sub_bytes >= 1)
        at++;
    return par_pack(at * 8, 0, 0);
}

struct ParLane {
    uint64_t exit;      // the state at the first symbol boundary at or behind the subsequence's end
    uint32_t n_begin;   // blocks whose DC code begins in the subsequence
    uint32_t dc_sum[3]; // the sum of their DC differences per component, modulo 2^32
    uint32_t fault;     // STRICT: the first fault's reason, R_OK without one
};

// Subsequence i from `entry`.  STRICT: first_block is the number of the first block that begins here, pred[c] the DC
// prediction it finds (both from the exclusive sums over the lanes before), coef the file's coefficients (int16,
// total_blocks * 64, undequantised, natural order): stores go to blocks below total_blocks only, and the lane is done
// when it reaches a block at or behind that.  Every trip consumes at least one bit; the trips are bounded by the
// subsequence's bits whatever the file holds.
template <bool STRICT, typename Src>
JD_HD void par_lane(const Src &src, const ParGeom &g, const Huff *dc, const Huff *ac, uint32_t i, uint64_t entry, uint32_t first_block,
                    const uint32_t *pred, int16_t *coef, ParLane &out)
{
    const uint64_t total_bits = (uint64_t)g.size * 8;
    const uint64_t end_byte = ((uint64_t)i + 1) * g.sub_bytes;
    const uint64_t end = (end_byte < g.size ? end_byte : g.size) * 8;
    uint64_t p = par_pos(entry);
    uint32_t b = par_blk(entry), k = par_k(entry);
    if (b >= g.blocks)
        b = 0; // (never: a state's block is below the MCU's count)
    uint32_t n_begin = 0, sums[3] = {0, 0, 0}, fault = R_OK;
    uint32_t cur = first_block - 1u; // the block being decoded (k > 0); wraps to none for a first lane's (never taken)
    int32_t dcv[3] = {0, 0, 0};
    if (STRICT)
        dcv[0] = (int32_t)pred[0], dcv[1] = (int32_t)pred[1], dcv[2] = (int32_t)pred[2];
    bool done = STRICT && k > 0 && cur >= g.total_blocks;
    for (uint32_t trip = 0; trip <= 8 * g.sub_bytes && p < end && !done; trip++) {
        const uint32_t c = b < g.luma_blocks ? 0u : b - g.luma_blocks + 1u; // 0, 1, 2
        if (STRICT && k == 0 && first_block + n_begin >= g.total_blocks)
            break; // what follows the last MCU is not looked at
        const ParWin w = par_window(src, g.size, p);
        const uint32_t o = (uint32_t)(p & 7);
        uint32_t len = 0, sym = 0;
        if (!par_lookup(k == 0 ? dc[c < 3 ? c : 0] : ac[c < 3 ? c : 0], par_peek(w, o, 16), len, sym)) {
            if (par_advance(w, p, 16) > total_bits) { // fewer than 16 bits left
                fault = R_EXHAUSTED, p = total_bits;
                break;
            }
            if (STRICT) {
                fault = R_BAD_CODE;
                break;
            }
            p = par_advance(w, p, 1);
            continue;
        }
        const uint64_t behind = par_advance(w, p, len);
        if (behind > total_bits) {
            fault = R_EXHAUSTED, p = total_bits;
            break;
        }
        uint32_t s, k_at = 0;
        bool ends = false; // the block ends with this symbol
        if (k == 0) {
            s = sym;
            if (s > 11) {
                if (STRICT) {
                    fault = R_CATEGORY;
                    break;
                }
                s = 11;
            }
        } else {
            const uint32_t r = sym >> 4;
            s = sym & 15u;
            if (s) {
                k_at = k + r;
                if (k_at > 63) {
                    if (STRICT) {
                        fault = R_RUN_PAST_63;
                        break;
                    }
                    s = 0, ends = true;
                } else if (s > 10) {
                    if (STRICT) {
                        fault = R_CATEGORY;
                        break;
                    }
                    s = 10;
                }
            } else if (r == 15) {
                k_at = k + 15;
                if (k_at > 63) {
                    if (STRICT) {
                        fault = R_RUN_PAST_63;
                        break;
                    }
                    ends = true;
                }
            } else if (r == 0) {
                ends = true;
            } else {
                if (STRICT) {
                    fault = R_BAD_SYMBOL;
                    break;
                }
                ends = true;
            }
        }
        uint64_t next = behind;
        int value = 0;
        if (s) {
            uint32_t v;
            if (o + len + s < 32) {
                v = par_peek(w, o + len, s);
                next = par_advance(w, p, len + s);
            } else { // the window again, from behind the code
                const ParWin w2 = par_window(src, g.size, behind);
                v = par_peek(w2, (uint32_t)(behind & 7), s);
                next = par_advance(w2, behind, s);
            }
            if (next > total_bits) {
                fault = R_EXHAUSTED, p = total_bits;
                break;
            }
            value = extend(v, s);
        }
        p = next;
        if (k == 0) {
            cur = first_block + n_begin;
            n_begin++;
            sums[c] += (uint32_t)value;
            if (STRICT) {
                dcv[c] = (int32_t)((uint32_t)dcv[c] + (uint32_t)value);
                if (dcv[c] < -2047 || dcv[c] > 2047) {
                    fault = R_DC_RANGE;
                    break;
                }
                if (cur < g.total_blocks)
                    coef[(size_t)cur * 64] = (int16_t)dcv[c];
            }
            k = 1;
        } else if (!ends) {
            if (STRICT && s && cur < g.total_blocks)
                coef[(size_t)cur * 64 + ZIGZAG[k_at & 63u]] = (int16_t)value;
            k = k_at + 1;
            ends = k > 63;
        }
        if (ends) {
            k = 0;
            b = b + 1 < g.blocks ? b + 1 : 0;
        }
    }
    // the data ends inside a block of the picture
    if (STRICT && fault == R_OK && p >= total_bits && k > 0 && cur < g.total_blocks)
        fault = R_EXHAUSTED;
    out.exit = par_pack(p, b, k & 63u);
    out.n_begin = n_begin;
    out.dc_sum[0] = sums[0], out.dc_sum[1] = sums[1], out.dc_sum[2] = sums[2];
    out.fault = STRICT ? fault : (uint32_t)R_OK;
}

} // namespace jpegdec
} // namespace tf
