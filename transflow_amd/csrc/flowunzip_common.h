// Flow archive members inflated on the device (flowunzip.hip): the part of a band's decoder that decides what is in
// bounds -- the bit reader, the block headers, the code tables, the per-symbol step and the state machine that strings
// them together -- as host/device inline functions over plain memory.  The kernel runs them in one lane of a wave over
// LDS; tools/flowunzip_host_check.cpp runs the same functions on the CPU under the sanitizers (DESIGN.md section 18;
// tests/flowunzip_ref.py is the Python statement of the same rules).
//
// A band is a byte range of a raw deflate stream that must inflate, on its own, to exactly `out_bytes` bytes: RFC 1951
// blocks with BFINAL 0, the last of which ends on the range's last bit.  Everything else is a rejection (Reject).
//
// The machine (`advance`) does by itself whatever one thread can do cheaply -- headers, tables, literals -- and hands
// its caller the rest as actions: refill the compressed window, copy a match inside the ring, copy stored bytes into
// the ring, flush the ring's new bytes to their destination.  Before it returns an action it has already checked the
// action's ranges; the caller checks them once more where it touches memory the band does not own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "deflate_tables.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FU_HD __host__ __device__ inline
#else
#define FU_HD inline
#endif

namespace tf {
namespace flowunzip {

using namespace deflate;

// why a band was rejected (0: it was not); the names are tests/flowunzip_ref.py's
enum Reject : uint32_t {
    R_OK = 0,
    R_BFINAL = 1,       // a block with BFINAL set
    R_BTYPE = 2,        // block type 3
    R_STORED_LEN = 3,   // LEN != ~NLEN
    R_BAD_CODE = 4,     // an over-subscribed or incomplete code, no end-of-block code, bits that are no code
    R_REPEAT_FIRST = 5, // repeat code 16 with no length before it
    R_REPEAT_PAST = 6,  // a repeat that runs past HLIT + HDIST
    R_BAD_SYMBOL = 7,   // literal/length symbol 286 / 287, distance symbol 30 / 31, HLIT > 286, HDIST > 30
    R_DISTANCE = 8,     // a distance beyond the bytes the band has produced
    R_OVERRUN = 9,      // output beyond the band's range
    R_SHORT = 10,       // the range's last block ended and bytes are missing
    R_EXHAUSTED = 11,   // the range ended inside a block
};

constexpr uint32_t RING_BYTES = 32768;     // the band's last 32768 bytes: every distance deflate can code
constexpr uint32_t RING_MASK = RING_BYTES - 1;
constexpr uint32_t WINDOW_BYTES = 1024;    // compressed bytes in reach of the bit reader
constexpr uint32_t SYMBOL_MARGIN = 16;     // a length/distance pair: 48 bits, and the 8 bytes the reader runs ahead
constexpr uint32_t FLUSH_AT = 2048;        // ring bytes not yet at their destination before a flush is asked for
constexpr uint32_t STORED_CHUNK = 1024;    // stored bytes per action
constexpr int FAST_BITS = 10;
constexpr int MAX_BITS = 15;
constexpr int N_LITLEN = 288, N_DIST = 32, MAX_LENGTHS = 320;
// A dynamic header is 14 bits, 19 * 3 bits, and at most 316 code-length symbols of at most 7 + 7 bits: 4495 bits, 562
// bytes.  The margin is asked for per part (read_dynamic is called with the window holding HEADER_WINDOW bytes ahead).
constexpr uint32_t HEADER_WINDOW = 600;
static_assert(HEADER_WINDOW + 8 <= WINDOW_BYTES, "a dynamic header must fit the window");
static_assert(FLUSH_AT + STORED_CHUNK + 258 < RING_BYTES, "the ring must hold what is not flushed");

// ---- the bit reader: bytes [0, size) of the band's range, of which win[0 .. win_len) holds those from win_base on -------
struct Bits {
    const uint8_t *win;
    uint32_t win_base, win_len;
    uint32_t size; // the band's compressed bytes
    uint32_t next; // the next byte of the range to take into buf
    uint64_t buf;  // cnt bits, the stream's next bit in bit 0
    uint32_t cnt;
};

FU_HD uint64_t bits_consumed(const Bits &b) { return 8ull * b.next - b.cnt; }

// whether `margin` bytes from the reader's place on are in the window (or the window reaches the range's end)
FU_HD bool need_refill(const Bits &b, uint32_t margin)
{
    const uint64_t have = (uint64_t)b.win_base + b.win_len;
    return have < b.size && (uint64_t)b.next + margin > have;
}

// at least 32 bits in buf afterwards (a caller needs 16 at the most), or every bit the range has left
FU_HD void fill(Bits &b)
{
    if (b.cnt >= 32)
        return;
    // four bytes at once where the window has them: four loads that do not wait for one another
    if (b.next - b.win_base < b.win_len && b.win_len - (b.next - b.win_base) >= 4) {
        const uint8_t *p = b.win + (b.next - b.win_base); // (win_base + win_len <= size: these are bytes of the range)
        const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        b.buf |= (uint64_t)v << b.cnt;
        b.cnt += 32;
        b.next += 4;
        return;
    }
    while (b.cnt <= 56 && b.next < b.size) {
        const uint32_t k = b.next - b.win_base; // (next >= win_base: the window only moves to `next`)
        if (k >= b.win_len)
            break;
        b.buf |= (uint64_t)b.win[k] << b.cnt;
        b.cnt += 8;
        b.next++;
    }
}

FU_HD void drop(Bits &b, uint32_t n) // n <= cnt
{
    b.buf >>= n;
    b.cnt -= n;
}

// n <= 16 bits, or false: the range has fewer left
FU_HD bool take(Bits &b, uint32_t n, uint32_t &v)
{
    fill(b);
    if (b.cnt < n)
        return false;
    v = (uint32_t)(b.buf & ((1ull << n) - 1));
    drop(b, n);
    return true;
}

// ---- a canonical code: count[len] symbols of each length, the symbols in code order, and for the codes of up to
// FAST_BITS bits a table by the next bits of the stream: (len << 9) | symbol, 0 where no such code starts
struct alignas(16) Code {
    uint16_t count[MAX_BITS + 1];
    uint16_t offs[MAX_BITS + 1];
    uint16_t symbol[N_LITLEN];
    uint16_t fast[1 << FAST_BITS];
};

FU_HD uint32_t reverse_code(uint32_t code, int len)
{
    uint32_t r = 0;
    for (int i = 0; i < len; i++)
        r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// lengths[n] (each <= 15, n <= 288) -> the code.  0: complete (or no symbol at all), > 0: incomplete by that many
// codes of 15 bits, < 0: over-subscribed (the table is then not to be used).
FU_HD int build_code(Code &c, const uint8_t *lengths, int n)
{
    for (int i = 0; i <= MAX_BITS; i++)
        c.count[i] = 0;
    for (int i = 0; i < (1 << FAST_BITS); i++)
        c.fast[i] = 0;
    for (int s = 0; s < n; s++)
        c.count[lengths[s] & 15]++;
    if (c.count[0] == n)
        return 0;
    int left = 1;
    for (int len = 1; len <= MAX_BITS; len++) {
        left <<= 1;
        left -= c.count[len];
        if (left < 0)
            return left;
    }
    c.offs[1] = 0;
    for (int len = 1; len < MAX_BITS; len++)
        c.offs[len + 1] = (uint16_t)(c.offs[len] + c.count[len]);
    for (int s = 0; s < n; s++) {
        const int len = lengths[s] & 15;
        if (len)
            c.symbol[c.offs[len]++] = (uint16_t)s; // (offs[len] < n: the counts sum to at most n)
    }
    uint32_t code = 0, index = 0;
    for (int len = 1; len <= FAST_BITS; len++) {
        const uint32_t cnt = c.count[len];
        for (uint32_t k = 0; k < cnt; k++) {
            const uint32_t entry = ((uint32_t)len << 9) | c.symbol[index + k];
            for (uint32_t j = reverse_code(code + k, len); j < (1u << FAST_BITS); j += 1u << len)
                c.fast[j] = (uint16_t)entry;
        }
        index += cnt;
        code = (code + cnt) << 1;
    }
    return left;
}

// the next symbol: R_OK, R_EXHAUSTED (the range ends inside the code) or R_BAD_CODE (15 bits that are no code)
FU_HD uint32_t decode(Bits &b, const Code &c, uint32_t &sym)
{
    fill(b);
    const uint32_t e = c.fast[b.buf & ((1u << FAST_BITS) - 1)];
    if (e) {
        const uint32_t len = e >> 9;
        if (len > b.cnt)
            return R_EXHAUSTED;
        drop(b, len);
        sym = e & 511u;
        return R_OK;
    }
    // a code longer than the table's: the counts in one go (loads that do not wait for one another), then bit by bit
    uint16_t count[MAX_BITS + 1];
    __builtin_memcpy(count, c.count, sizeof(count));
    int code = 0, first = 0, index = 0;
    uint32_t bits = (uint32_t)b.buf;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int len = 1; len <= MAX_BITS; len++) {
        if ((uint32_t)len > b.cnt)
            return R_EXHAUSTED;
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int n = count[len];
        if (code - n < first) {
            const int at = index + (code - first);
            if (at < 0 || at >= N_LITLEN)
                return R_BAD_CODE; // (never: the counts come from at most 288 lengths)
            sym = c.symbol[at];
            drop(b, (uint32_t)len);
            return R_OK;
        }
        index += n;
        first += n;
        first <<= 1;
        code <<= 1;
    }
    return R_BAD_CODE;
}

// ---- the block headers -------------------------------------------------------------------------------------------------
FU_HD uint32_t read_block_header(Bits &b, uint32_t &type)
{
    uint32_t v;
    if (!take(b, 3, v))
        return R_EXHAUSTED;
    if (v & 1u)
        return R_BFINAL;
    type = v >> 1;
    return type == 3 ? R_BTYPE : R_OK;
}

// behind a stored block's header: to the byte boundary, LEN, NLEN.  `src` is where the block's bytes begin in the
// range; the reader is left empty and placed there.
FU_HD uint32_t read_stored(Bits &b, uint32_t &len, uint32_t &src)
{
    uint32_t a, n;
    drop(b, b.cnt & 7u);
    if (!take(b, 16, a) || !take(b, 16, n))
        return R_EXHAUSTED;
    if (a != (~n & 0xFFFFu))
        return R_STORED_LEN;
    len = a;
    src = b.next - b.cnt / 8; // (cnt is a multiple of 8 here)
    b.next = src;
    b.buf = 0;
    b.cnt = 0;
    return R_OK;
}

FU_HD void build_fixed(Code &lit, Code &dist, uint8_t *lengths)
{
    for (int s = 0; s < N_LITLEN; s++)
        lengths[s] = (uint8_t)(s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8)));
    build_code(lit, lengths, N_LITLEN);
    for (int s = 0; s < N_DIST; s++)
        lengths[s] = 5;
    build_code(dist, lengths, N_DIST);
}

// a dynamic block's header; lengths: MAX_LENGTHS bytes of working space
FU_HD uint32_t read_dynamic(Bits &b, Code &lit, Code &dist, uint8_t *lengths)
{
    uint32_t v;
    if (!take(b, 14, v))
        return R_EXHAUSTED;
    const uint32_t nlen = (v & 31u) + 257, ndist = ((v >> 5) & 31u) + 1, ncode = (v >> 10) + 4;
    if (nlen > 286 || ndist > 30)
        return R_BAD_SYMBOL;
    for (int i = 0; i < 19; i++)
        lengths[i] = 0;
    for (uint32_t i = 0; i < ncode; i++) {
        if (!take(b, 3, v))
            return R_EXHAUSTED;
        lengths[CLEN_ORDER[i]] = (uint8_t)v;
    }
    if (build_code(lit, lengths, 19) != 0) // the code-length code, in the literal code's place for now
        return R_BAD_CODE;
    if (lit.count[0] == 19)
        return R_BAD_CODE;
    const uint32_t total = nlen + ndist; // <= 316
    uint32_t index = 0;
    while (index < total) {
        uint32_t sym;
        const uint32_t rc = decode(b, lit, sym);
        if (rc != R_OK)
            return rc;
        if (sym < 16) {
            lengths[index++] = (uint8_t)sym;
            continue;
        }
        uint32_t value = 0, repeat;
        if (sym == 16) {
            if (index == 0)
                return R_REPEAT_FIRST;
            value = lengths[index - 1];
            if (!take(b, 2, v))
                return R_EXHAUSTED;
            repeat = 3 + v;
        } else if (sym == 17) {
            if (!take(b, 3, v))
                return R_EXHAUSTED;
            repeat = 3 + v;
        } else if (sym == 18) {
            if (!take(b, 7, v))
                return R_EXHAUSTED;
            repeat = 11 + v;
        } else {
            return R_BAD_CODE; // (never: the code has 19 symbols)
        }
        if (index + repeat > total)
            return R_REPEAT_PAST;
        while (repeat--)
            lengths[index++] = (uint8_t)value;
    }
    if (lengths[256] == 0)
        return R_BAD_CODE;
    // the distance lengths first: the literal code's construction overwrites nothing of `lengths`, but the literal
    // table still holds the code-length code until it is built
    const int derr = build_code(dist, lengths + nlen, (int)ndist);
    if (derr < 0 || (derr > 0 && !(dist.count[1] == 1 && dist.count[0] == ndist - 1)))
        return R_BAD_CODE;
    if (build_code(lit, lengths, (int)nlen) != 0)
        return R_BAD_CODE;
    return R_OK;
}

// ---- one symbol of a coded block -----------------------------------------------------------------------------------------
enum TokenKind : uint32_t { T_LITERAL = 0, T_END = 1, T_MATCH = 2 };
struct Token {
    uint32_t kind, value, distance; // value: the literal, or the match's length
};

// produced: the bytes the band has made so far; out_bytes: what it must make
FU_HD uint32_t step(Bits &b, const Code &lit, const Code &dist, uint32_t produced, uint32_t out_bytes, Token &t)
{
    uint32_t sym, v;
    uint32_t rc = decode(b, lit, sym);
    if (rc != R_OK)
        return rc;
    if (sym < 256) {
        if (produced >= out_bytes)
            return R_OVERRUN;
        t.kind = T_LITERAL, t.value = sym, t.distance = 0;
        return R_OK;
    }
    if (sym == 256) {
        t.kind = T_END, t.value = 0, t.distance = 0;
        return R_OK;
    }
    if (sym >= 286)
        return R_BAD_SYMBOL;
    const uint32_t k = sym - 257;
    if (!take(b, LENGTH_EXTRA[k], v))
        return R_EXHAUSTED;
    const uint32_t len = LENGTH_BASE[k] + v;
    rc = decode(b, dist, sym);
    if (rc != R_OK)
        return rc;
    if (sym >= 30)
        return R_BAD_SYMBOL;
    if (!take(b, DIST_EXTRA[sym], v))
        return R_EXHAUSTED;
    const uint32_t d = DIST_BASE[sym] + v;
    if (d > produced)
        return R_DISTANCE;
    if (len > out_bytes - produced) // (produced <= out_bytes always)
        return R_OVERRUN;
    t.kind = T_MATCH, t.value = len, t.distance = d;
    return R_OK;
}

// ---- the machine -------------------------------------------------------------------------------------------------------
enum Phase : uint32_t { P_HEADER = 0, P_SYMBOLS = 1, P_STORED = 2 };
enum ActionKind : uint32_t {
    A_DONE = 0,   // a: the Reject (R_OK: the band is whole; flush what is left)
    A_REFILL = 1, // the window becomes bytes [a, a + b) of the range
    A_MATCH = 2,  // ring bytes [a, a + b) become copies of the bytes c back, in order (c <= a, c <= 32768, b <= 258)
    A_STORED = 3, // ring bytes [a, a + b) become bytes [c, c + b) of the range
    A_FLUSH = 4,  // ring bytes [flushed, produced rounded down to 64) go to their destination
};
struct Action {
    uint32_t kind, a, b, c;
};

struct State {
    Bits bits;
    uint32_t phase;
    uint32_t produced, out_bytes, flushed;
    uint32_t stored_left, stored_src;
    uint32_t tables_fixed; // the tables hold the fixed codes: a run of fixed blocks builds them once
};

FU_HD void start(State &s, const uint8_t *win, uint32_t size, uint32_t out_bytes)
{
    s.bits.win = win, s.bits.win_base = 0, s.bits.win_len = 0, s.bits.size = size, s.bits.next = 0, s.bits.buf = 0, s.bits.cnt = 0;
    s.phase = P_HEADER, s.produced = 0, s.out_bytes = out_bytes, s.flushed = 0, s.stored_left = 0, s.stored_src = 0;
    s.tables_fixed = 0;
}

FU_HD Action make_action(uint32_t kind, uint32_t a, uint32_t b, uint32_t c)
{
    Action x;
    x.kind = kind, x.a = a, x.b = b, x.c = c;
    return x;
}

FU_HD Action refill_action(State &s)
{
    Bits &b = s.bits;
    b.win_base = b.next; // (next <= size)
    b.win_len = b.size - b.next < WINDOW_BYTES ? b.size - b.next : WINDOW_BYTES;
    return make_action(A_REFILL, b.win_base, b.win_len, 0);
}

// Runs until the caller has to do something.  Every trip takes at least one bit of the range or returns, so the trips
// are bounded by the range's bits.  ring: RING_BYTES; lengths: MAX_LENGTHS.
FU_HD Action advance(State &s, Code &lit, Code &dist, uint8_t *lengths, uint8_t *ring)
{
    Bits &b = s.bits;
    for (;;) {
        if (s.produced - s.flushed >= FLUSH_AT)
            return make_action(A_FLUSH, 0, 0, 0);
        if (s.phase == P_HEADER) {
            if (bits_consumed(b) == 8ull * b.size)
                return make_action(A_DONE, s.produced == s.out_bytes ? R_OK : R_SHORT, 0, 0);
            if (need_refill(b, HEADER_WINDOW))
                return refill_action(s);
            uint32_t type = 0;
            uint32_t rc = read_block_header(b, type);
            if (rc != R_OK)
                return make_action(A_DONE, rc, 0, 0);
            if (type == 0) {
                uint32_t len = 0, src = 0;
                rc = read_stored(b, len, src);
                if (rc != R_OK)
                    return make_action(A_DONE, rc, 0, 0);
                if (len > b.size - src) // (src <= size)
                    return make_action(A_DONE, R_EXHAUSTED, 0, 0);
                if (len > s.out_bytes - s.produced)
                    return make_action(A_DONE, R_OVERRUN, 0, 0);
                s.stored_left = len, s.stored_src = src, s.phase = P_STORED;
            } else if (type == 1) {
                if (!s.tables_fixed)
                    build_fixed(lit, dist, lengths);
                s.tables_fixed = 1;
                s.phase = P_SYMBOLS;
            } else {
                s.tables_fixed = 0; // (whether or not the header is read to its end)
                rc = read_dynamic(b, lit, dist, lengths);
                if (rc != R_OK)
                    return make_action(A_DONE, rc, 0, 0);
                s.phase = P_SYMBOLS;
            }
        } else if (s.phase == P_STORED) {
            if (s.stored_left == 0) {
                s.phase = P_HEADER;
                continue;
            }
            const uint32_t n = s.stored_left < STORED_CHUNK ? s.stored_left : STORED_CHUNK;
            const Action x = make_action(A_STORED, s.produced, n, s.stored_src);
            s.produced += n, s.stored_src += n, s.stored_left -= n;
            b.next = s.stored_src;
            return x;
        } else {
            if (need_refill(b, SYMBOL_MARGIN))
                return refill_action(s);
            Token t;
            const uint32_t rc = step(b, lit, dist, s.produced, s.out_bytes, t);
            if (rc != R_OK)
                return make_action(A_DONE, rc, 0, 0);
            if (t.kind == T_LITERAL) {
                ring[s.produced & RING_MASK] = (uint8_t)t.value;
                s.produced++;
            } else if (t.kind == T_END) {
                s.phase = P_HEADER;
            } else {
                const Action x = make_action(A_MATCH, s.produced, t.value, t.distance);
                s.produced += t.value;
                return x;
            }
        }
    }
}

} // namespace flowunzip
} // namespace tf
