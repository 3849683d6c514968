// MT19937 as numpy's legacy RandomState runs it, stated on word positions: the raw (untempered) word stream x[k] obeys
//   x[k + 624] = x[k + 397] ^ twist(x[k], x[k + 1])          at every k,
// so any 624 consecutive raw words are a state, and (key = x[P .. P + 623], pos = 0) handed to numpy.random.set_state
// continues the stream from word P.  Shared by mt19937.hip (the kernels' per-word statements, the handle's host side) and
// tools/mt_host_check.cpp (the same host code under the sanitizers).  Nothing here is a pasted table: the characteristic
// polynomial comes out of Berlekamp-Massey over the generator's own output, the jump polynomials out of t^J mod it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define TF_MT_HD __host__ __device__
#else
#define TF_MT_HD
#endif

namespace tf {
namespace mt {

constexpr int NW = 624, MW = 397;        // words of a state; the recurrence's middle tap
constexpr int DEG = 19937;               // bits of a state = degree of the characteristic polynomial
constexpr int PREFIX = DEG + NW - 1;     // raw words from a state that one jump reads: x[i + j], i < DEG, j < NW
constexpr int POLY_WORDS = (DEG + 63) / 64; // 64-bit words of a polynomial of degree < DEG
constexpr uint32_t UPPER = 0x80000000u, LOWER = 0x7fffffffu, MAG = 0x9908b0dfu;

// x[k + 624] from a = x[k], b = x[k + 1], c = x[k + 397]
TF_MT_HD inline uint32_t next_word(uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t y = (a & UPPER) | (b & LOWER);
    return c ^ (y >> 1) ^ ((b & 1u) ? MAG : 0u);
}

TF_MT_HD inline uint32_t temper(uint32_t y)
{
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// numpy's double from two consecutive tempered words: ((a >> 5) * 2^26 + (b >> 6)) / 2^53.  The 53-bit integer and its
// scaling by a power of two are exact in double.
TF_MT_HD inline double to_double(uint32_t a, uint32_t b)
{
    const uint64_t v = ((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6);
    return (double)v * (1.0 / 9007199254740992.0);
}

// The state a seed gives (init_genrand; numpy.random.seed of an integer): key[0] = seed, pos = 624.
inline void seed_key(uint32_t seed, uint32_t *key)
{
    key[0] = seed;
    for (uint32_t i = 1; i < (uint32_t)NW; i++)
        key[i] = 1812433253u * (key[i - 1] ^ (key[i - 1] >> 30)) + i;
}

// x[0 .. count) from x[0 .. 624) = key (count >= 624: out holds count words)
inline void raw_stream(const uint32_t *key, size_t count, uint32_t *out)
{
    for (size_t k = 0; k < count; k++)
        out[k] = k < (size_t)NW ? key[k] : next_word(out[k - NW], out[k - NW + 1], out[k - NW + MW]);
}

// The window x[pos .. pos + 623] of the stream whose first 624 words are key: what (key, pos) of numpy's state tuple
// means once pos words of the block have been handed out (pos = 624: the whole next block).
inline void window_at(const uint32_t *key, int pos, uint32_t *win)
{
    std::vector<uint32_t> x((size_t)NW + (size_t)pos);
    raw_stream(key, x.size(), x.data());
    for (int j = 0; j < NW; j++)
        win[j] = x[(size_t)pos + j];
}

// Only the top bit of a window's first word takes part in the recurrence: a seeded key's word 0 is the seed itself, no
// word the recurrence would have produced, and the polynomial relations (which hold for produced words) fail on its low
// 31 bits.  The word the recurrence would have put there follows from x[623] = x[396] ^ twist(x[-1], x[0]).
inline uint32_t canonical_word0(const uint32_t *win)
{
    const uint32_t t = win[NW - 1] ^ win[MW - 1];
    const uint32_t low = t >> 31;
    const uint32_t u = t ^ (low ? MAG : 0u);
    return (win[0] & UPPER) | ((u << 1) & 0x7ffffffeu) | low;
}

// ---- GF(2) polynomials: bit i of word i / 64 is the coefficient of t^i ------------------------------------------------
typedef std::vector<uint64_t> Poly;

inline bool poly_bit(const Poly &p, size_t i) { return i / 64 < p.size() && ((p[i / 64] >> (i % 64)) & 1u); }
inline void poly_flip(Poly &p, size_t i) { p[i / 64] ^= (uint64_t)1 << (i % 64); }

inline int poly_degree(const Poly &p)
{
    for (size_t w = p.size(); w-- > 0;)
        if (p[w])
            return (int)(w * 64 + 63 - (size_t)__builtin_clzll(p[w]));
    return -1;
}

inline size_t poly_weight(const Poly &p)
{
    size_t n = 0;
    for (uint64_t w : p)
        n += (size_t)__builtin_popcountll(w);
    return n;
}

// dst ^= src << shift; dst is long enough for every set bit
inline void poly_xor_shifted(Poly &dst, const Poly &src, size_t shift)
{
    const size_t ws = shift / 64, bs = shift % 64;
    for (size_t w = 0; w < src.size(); w++) {
        if (!src[w])
            continue;
        dst[w + ws] ^= src[w] << bs;
        if (bs && w + ws + 1 < dst.size())
            dst[w + ws + 1] ^= src[w] >> (64 - bs);
    }
}

// Berlekamp-Massey over GF(2): the shortest linear recurrence of bits[0 .. n).  Returns its length L and the connection
// polynomial C (C_0 = 1): bits[k] = XOR over i = 1 .. L of C_i bits[k - i].
inline int berlekamp_massey(const std::vector<uint8_t> &bits, Poly &conn)
{
    const size_t n = bits.size(), words = n / 64 + 2;
    Poly C(words, 0), B(words, 0), T, R(words, 0); // R: bit i = bits[k - i], the sequence read backwards from k
    C[0] = B[0] = 1;
    size_t L = 0, m = 1;
    for (size_t k = 0; k < n; k++) {
        uint64_t carry = bits[k] & 1u;
        const size_t live = k / 64 + 1;
        for (size_t w = 0; w < live; w++) {
            const uint64_t next = R[w] >> 63;
            R[w] = (R[w] << 1) | carry;
            carry = next;
        }
        uint64_t d = 0;
        for (size_t w = 0; w <= L / 64; w++)
            d ^= C[w] & R[w];
        if (!(__builtin_popcountll(d) & 1)) {
            m++;
        } else if (2 * L <= k) {
            T = C;
            poly_xor_shifted(C, B, m);
            L = k + 1 - L;
            B.swap(T);
            m = 1;
        } else {
            poly_xor_shifted(C, B, m);
            m++;
        }
    }
    conn.swap(C);
    return (int)L;
}

// The characteristic polynomial of the recurrence, from 2 * DEG + 64 low bits of a seeded generator's tempered words:
// phi_i = C_(L - i), so that XOR over i of phi_i x[k + i] = 0 for produced words.  Returns its degree (DEG, or the
// caller has found a bug); terms: the exponents of its set coefficients, ascending.
inline int characteristic_polynomial(Poly &phi, std::vector<uint32_t> &terms)
{
    const size_t n = 2 * (size_t)DEG + 64;
    std::vector<uint32_t> key(NW), x(n + NW);
    seed_key(5489u, key.data());
    raw_stream(key.data(), x.size(), x.data());
    std::vector<uint8_t> bits(n);
    for (size_t k = 0; k < n; k++)
        bits[k] = (uint8_t)(temper(x[k + NW]) & 1u);
    Poly conn;
    const int L = berlekamp_massey(bits, conn);
    phi.assign((size_t)L / 64 + 1, 0);
    terms.clear();
    for (int i = 0; i <= L; i++)
        if (poly_bit(conn, (size_t)(L - i))) {
            poly_flip(phi, (size_t)i);
            terms.push_back((uint32_t)i);
        }
    return L;
}

// p (degree < 2 * DEG, 2 * POLY_WORDS + 1 words) reduced modulo phi in place, phi given by its terms (the last is DEG)
inline void poly_reduce(Poly &p, const std::vector<uint32_t> &terms)
{
    for (int d = poly_degree(p); d >= DEG; d--) {
        if (!poly_bit(p, (size_t)d))
            continue;
        for (uint32_t e : terms)
            poly_flip(p, (size_t)d - (size_t)DEG + e);
    }
}

// t^J mod phi, POLY_WORDS words: square-and-multiply from J's top bit down.  Squaring over GF(2) spreads the bits.
inline void jump_polynomial(uint64_t J, const std::vector<uint32_t> &terms, Poly &out)
{
    Poly r(2 * (size_t)POLY_WORDS + 1, 0), sq(2 * (size_t)POLY_WORDS + 1, 0);
    r[0] = 1;
    for (int b = 63; b >= 0; b--) {
        std::fill(sq.begin(), sq.end(), 0);
        for (int i = poly_degree(r); i >= 0; i--)
            if (poly_bit(r, (size_t)i))
                poly_flip(sq, 2 * (size_t)i);
        poly_reduce(sq, terms);
        r.swap(sq);
        if ((J >> b) & 1u) {
            std::fill(sq.begin(), sq.end(), 0);
            poly_xor_shifted(sq, r, 1);
            poly_reduce(sq, terms);
            r.swap(sq);
        }
    }
    out.assign(r.begin(), r.begin() + POLY_WORDS);
}

// The exponents of a polynomial's set coefficients, ascending (what the jump kernel walks)
inline void poly_terms(const uint64_t *poly, std::vector<uint32_t> &terms)
{
    terms.clear();
    for (int i = 0; i < DEG; i++)
        if ((poly[i / 64] >> (i % 64)) & 1u)
            terms.push_back((uint32_t)i);
}

// out[j] = XOR over the set coefficients i of poly of x[i + j], j < 624, x the stream from key (its word 0 made the
// recurrence's own first): with poly = t^J mod phi and J >= 1 that is x[J .. J + 623].
inline void apply_polynomial(const uint64_t *poly, const uint32_t *key, uint32_t *out)
{
    std::vector<uint32_t> x(PREFIX), terms;
    raw_stream(key, x.size(), x.data());
    x[0] = canonical_word0(key);
    poly_terms(poly, terms);
    for (int j = 0; j < NW; j++) {
        uint32_t acc = 0;
        for (uint32_t i : terms)
            acc ^= x[(size_t)i + (size_t)j];
        out[j] = acc;
    }
}

// RandomState.random_sample on the CPU, in numpy's own block form: key is regenerated 624 words at a time when pos
// reaches 624.  key and pos are updated as numpy updates them.
inline void random_sample_blocks(uint32_t *key, int *pos, size_t n, double *out)
{
    auto word = [&]() -> uint32_t {
        if (*pos >= NW) {
            uint32_t nxt[NW];
            for (int k = 0; k < NW; k++) {
                const uint32_t b = k + 1 < NW ? key[k + 1] : nxt[0];
                const uint32_t c = k + MW < NW ? key[k + MW] : nxt[k + MW - NW];
                nxt[k] = next_word(key[k], b, c);
            }
            for (int k = 0; k < NW; k++)
                key[k] = nxt[k];
            *pos = 0;
        }
        return temper(key[(*pos)++]);
    };
    for (size_t i = 0; i < n; i++) {
        const uint32_t a = word(), b = word();
        out[i] = to_double(a, b);
    }
}

} // namespace mt
} // namespace tf
