// The frame's own Huffman tables (jpeg.hip, mode 1): libjpeg's jpeg_gen_optimal_table (jchuff.c) as code that the host
// and one thread of the device run alike, and jpeg_make_c_derived_tbl behind it.  tools/jpeg_huff_host_check.cpp runs
// this file on the CPU; tests/jpeg_ref.py is the numpy statement of the same rule.
//
// The rule: 257 frequencies, the last a reserved symbol of frequency 1 so that no real code is all ones.  Until only
// one is left, the two smallest non-zero frequencies are merged -- among equals the LARGEST index is taken, first c1,
// then c2 over the rest (libjpeg scans upward with <=) -- and every symbol of the two merged trees gets one bit longer:
// the trees are the `others` chains, c2's linked behind c1's.  Code sizes above 32 are refused (JERR_HUFF_CLEN_OVERFLOW);
// sizes 17 to 32 are brought to 16 by moving pairs of symbols up under a shorter prefix; the reserved symbol then leaves
// the longest length.  The symbols are listed by (code size BEFORE that limiting, symbol).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JH_HD __host__ __device__ inline
#else
#define JH_HD inline
#endif

namespace tf {
namespace jpeg {

constexpr int HUFF_SYMS = 257;                  // 256 symbols and the reserved one
constexpr int HUFF_MAX_CLEN = 32;               // jchuff.c MAX_CLEN
constexpr uint32_t HUFF_SENTINEL = 1000000000u; // jchuff.c: a frequency above it is never selected
// 6 * 64 * n_mcus and the sum of a histogram stay at or below the sentinel: every frequency, merged ones included, is
// then selectable and no uint32_t sum wraps.

enum HuffFault { HUFF_OK = 0, HUFF_CLEN_OVERFLOW = 1, HUFF_EMPTY = 2 };

struct HuffWork {
    uint32_t freq[HUFF_SYMS];
    uint16_t codesize[HUFF_SYMS];
    int16_t others[HUFF_SYMS];
};

// the smallest non-zero frequency, the largest index among equals; `skip` is left out.  -1: none.
JH_HD int huff_pick(const uint32_t *freq, int skip)
{
    int c = -1;
    uint32_t v = HUFF_SENTINEL;
    for (int i = 0; i < HUFF_SYMS; i++)
        if (freq[i] && freq[i] <= v && i != skip)
            c = i, v = freq[i];
    return c;
}

// c2's tree joins c1's: one more bit for every symbol of both
JH_HD void huff_link(uint16_t *codesize, int16_t *others, int c1, int c2)
{
    codesize[c1]++;
    while (others[c1] >= 0)
        c1 = others[c1], codesize[c1]++;
    others[c1] = (int16_t)c2;
    codesize[c2]++;
    while (others[c2] >= 0)
        c2 = others[c2], codesize[c2]++;
}

// bits[1 .. 32], the symbols of every code size with the reserved one among them, brought to 16 bits at most; the
// reserved symbol leaves the longest length; bits16 is what DHT carries.  bits[0] and bits[33] are room, not counts.
JH_HD void huff_limit(int *bits, uint8_t *bits16)
{
    for (int i = HUFF_MAX_CLEN; i > 16; i--)
        while (bits[i] > 0) {
            int j = i - 2;
            while (j > 0 && bits[j] == 0) // (j > 0 always: the sizes are those of a full tree)
                j--;
            bits[i] -= 2, bits[i - 1]++, bits[j + 1] += 2, bits[j]--;
        }
    int i = 16;
    while (i > 0 && bits[i] == 0)
        i--;
    bits[i]--;
    for (int k = 0; k < 16; k++)
        bits16[k] = (uint8_t)bits[k + 1];
}

// code sizes -> the DHT's 16 counts and its symbols (at most 256; *n_vals of them).  vals needs room for 256.
JH_HD int huff_finish(const uint16_t *codesize, uint8_t *bits16, uint8_t *vals, int *n_vals)
{
    int bits[HUFF_MAX_CLEN + 2], offs[HUFF_MAX_CLEN + 2];
    for (int i = 0; i < HUFF_MAX_CLEN + 2; i++)
        bits[i] = 0, offs[i] = 0;
    for (int i = 0; i < 16; i++)
        bits16[i] = 0;
    *n_vals = 0;
    int used = 0;
    for (int i = 0; i < HUFF_SYMS; i++)
        if (codesize[i]) {
            if (codesize[i] > HUFF_MAX_CLEN)
                return HUFF_CLEN_OVERFLOW;
            bits[codesize[i]]++;
            if (i < 256)
                offs[codesize[i] + 1]++, used++;
        }
    if (!used)
        return HUFF_EMPTY; // (libjpeg's loops below would run off their array)
    for (int i = 1; i <= HUFF_MAX_CLEN + 1; i++) // offs[s]: the symbols with a shorter size
        offs[i] += offs[i - 1];
    for (int s = 0; s < 256; s++)
        if (codesize[s])
            vals[offs[codesize[s]]++] = (uint8_t)s;
    *n_vals = used;
    huff_limit(bits, bits16);
    return HUFF_OK;
}

// jpeg_gen_optimal_table.  w.freq[0 .. 255] hold the counts (they are used up); the rest of `w` is set here.
JH_HD int gen_optimal_table(HuffWork &w, uint8_t *bits16, uint8_t *vals, int *n_vals)
{
    w.freq[256] = 1;
    for (int i = 0; i < HUFF_SYMS; i++)
        w.codesize[i] = 0, w.others[i] = -1;
    for (;;) {
        const int c1 = huff_pick(w.freq, -1);
        const int c2 = huff_pick(w.freq, c1);
        if (c2 < 0)
            break;
        w.freq[c1] += w.freq[c2];
        w.freq[c2] = 0;
        huff_link(w.codesize, w.others, c1, c2);
    }
    return huff_finish(w.codesize, bits16, vals, n_vals);
}

// jchuff.c jpeg_make_c_derived_tbl: entries[symbol] = (length << 16) | code, 0 for a symbol the table does not have
JH_HD void huff_entries(const uint8_t *bits, const uint8_t *vals, uint32_t *entries, int n_entries)
{
    for (int s = 0; s < n_entries; s++)
        entries[s] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int c = 0; c < bits[len - 1]; c++, k++, code++)
            if (k < 256 && vals[k] < n_entries)
                entries[vals[k]] = ((uint32_t)len << 16) | code;
        code <<= 1;
    }
}

} // namespace jpeg
} // namespace tf
