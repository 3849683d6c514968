// PNG of a device-resident RGB frame: 8-bit colour type 2, no interlace, every row filtered with the type of the
// smallest sum of min(b, 256 - b), and a zlib stream cut into bands that are coded side by side (tests/png_ref.py is
// the numpy statement of the same rules).
//
// A band is `band_rows` rows of the filtered stream.  Its deflate data is one dynamic-Huffman block -- the table header
// is a constant of the library: a fixed literal/length code, a distance alphabet of the single code 0 -- and an empty
// stored block that brings the stream to a byte boundary, so a band's bytes depend on nothing but its own rows and the
// bands concatenate into one valid stream.  Matches are runs: distance 1, never across the band's first byte.
// With tf_png_set_code(enc, 1) the literal/length code is the frame's own, built from the tokens of all its bands, and a
// band whose coded form would not be smaller is stored instead (tests/png_frame_code_ref.py states that mode).
//
//   k_png_filter   one work-group per row: the five candidates' sums, the choice, the filtered row to HBM, and the
//                  row's two Adler sums (the plain sum and the sum weighted by the bytes behind, 64-bit, reduced once).
//   k_png_deflate  one wave per band, 64 bytes a trip.  A lane compares its byte with its left neighbour's; the ballot
//                  of equal lanes and the count carried from the trip before give it its place in a run.  A run leaves
//                  a match of 258 at the lane where the count reaches it, and what is left -- a match, or one or two
//                  literals -- at the lane behind its end, in front of that lane's own literal; the position one past
//                  the band is a lane too and its own symbol is end-of-block.  A wave prefix sum of the bit counts
//                  places the tokens in an LDS bit buffer that starts out holding the table header; after every trip
//                  its whole bytes go to the band's staging slot and the bits left over to its front.
//   k_png_count    (the frame's own code, tf_png_set_code) one wave per band: the same tokeniser, the tokens counted in
//                  LDS; the band's 286 counts go to its row.
//   k_png_total    (the same) the frame's histogram: the column sums of those rows.
//   k_png_table    (the same) one work-group: the code of the histogram (deflate_code.h), the entries and the header
//                  k_png_deflate reads, the bits each symbol costs.  k_png_deflate then adds up its band's counts x
//                  costs first, and where the coded form would not be smaller than the stored one it copies the band
//                  behind stored-block headers instead.
//   k_slot_scan    exclusive sum of the bands' chunk sizes, data + 12 (one work-group; stream_common.h).
//   k_png_pack     one wave per band writes length, "IDAT", the data and the chunk's CRC-32 at the band's offset: the
//                  lanes take contiguous slices through the byte table and the slices' CRCs are combined by
//                  multiplying with x^(8 * bytes behind) modulo the polynomial (crc32_common.h).  No byte at or past
//                  `capacity` is written.
#include "png_common.h"
#include "stream_common.h"

#include <cstring>

namespace tf {
namespace png {

constexpr uint32_t ADLER_BASE = 65521;

// ---- filter ----------------------------------------------------------------------------------------------------------
constexpr int FILTER_BLOCK = 256;

__device__ __forceinline__ int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int filter_byte(int type, int x, int a, int b, int c)
{
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x - pred) & 0xFF;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = WAVE / 2; d; d >>= 1)
        v += __shfl_xor(v, d, WAVE);
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int d = WAVE / 2; d; d >>= 1)
        v += __shfl_xor(v, d, WAVE);
    return v;
}

// rowsums[2 r], [2 r + 1]: sum of the filtered row's L = 1 + 3 W bytes, and sum of (L - j) byte[j], both mod 65521.
// Largest values: 255 L < 2^26 and 255 L (L + 1) / 2 < 2^43 for W = 65535, so nothing is reduced before the end.
__global__ __launch_bounds__(FILTER_BLOCK) void k_png_filter(const uint8_t *__restrict__ rgb, int W, uint8_t *__restrict__ filtered,
                                                             uint32_t *__restrict__ rowsums)
{
    __shared__ uint32_t s_cost[FILTER_BLOCK / WAVE][5];
    __shared__ unsigned long long s_adler[FILTER_BLOCK / WAVE][2];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int row = blockIdx.x, n = 3 * W;
    const uint8_t *cur = rgb + (size_t)row * n;
    const uint8_t *prev = row ? cur - n : nullptr;
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += FILTER_BLOCK) {
        const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = prev ? prev[i] : 0, c = (prev && i >= 3) ? prev[i - 3] : 0;
#pragma unroll
        for (int t = 0; t < 5; t++) {
            const int v = filter_byte(t, x, a, b, c);
            cost[t] += (uint32_t)min(v, 256 - v);
        }
    }
#pragma unroll
    for (int t = 0; t < 5; t++) {
        const uint32_t s = wave_sum(cost[t]);
        if (lane == 0)
            s_cost[wave][t] = s;
    }
    __syncthreads();
    int type = 0;
    uint32_t best = 0;
#pragma unroll
    for (int t = 0; t < 5; t++) {
        uint32_t s = 0;
        for (int w = 0; w < FILTER_BLOCK / WAVE; w++)
            s += s_cost[w][t];
        if (t == 0 || s < best) // ties stay with the lowest type
            best = s, type = t;
    }
    const size_t L = (size_t)n + 1;
    uint8_t *out = filtered + (size_t)row * L;
    unsigned long long s1 = 0, s2 = 0;
    if (tid == 0) {
        out[0] = (uint8_t)type;
        s1 = (unsigned long long)type, s2 = (unsigned long long)type * L;
    }
    for (int i = tid; i < n; i += FILTER_BLOCK) {
        const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = prev ? prev[i] : 0, c = (prev && i >= 3) ? prev[i - 3] : 0;
        const int v = filter_byte(type, x, a, b, c);
        out[1 + i] = (uint8_t)v;
        s1 += (unsigned long long)v;
        s2 += (unsigned long long)v * (L - 1 - (size_t)i);
    }
    s1 = wave_sum64(s1), s2 = wave_sum64(s2);
    if (lane == 0)
        s_adler[wave][0] = s1, s_adler[wave][1] = s2;
    __syncthreads();
    if (tid == 0) {
        s1 = s2 = 0;
        for (int w = 0; w < FILTER_BLOCK / WAVE; w++)
            s1 += s_adler[w][0], s2 += s_adler[w][1];
        rowsums[2 * row] = (uint32_t)(s1 % ADLER_BASE);
        rowsums[2 * row + 1] = (uint32_t)(s2 % ADLER_BASE);
    }
}

// ---- deflate ---------------------------------------------------------------------------------------------------------
struct DeflateArgs {
    const uint8_t *filtered; // H rows of row_bytes
    uint32_t row_bytes;
    int H, band_rows;
    const Tables *tables;    // the library's constant code, or what k_png_table made of the frame's histogram
    const uint32_t *counts;  // null, or per band its 286 token counts: a band that would not shrink is stored
    const FrameCode *code;   // with counts: the bits each symbol costs
    uint8_t *staging;        // n_bands slots of slot_bytes
    uint32_t slot_bytes;
    uint32_t *lengths;       // per band: the bytes it wrote
    uint32_t *overflow;      // set if a band had more bytes than its slot (the bound of png_common.h says: never)
};

constexpr int TRIPS = 4;

// What the lane of band byte i emits in a trip, in stream order: a match of `match` bytes, or `pending` (0 - 2) literals
// of its left neighbour's byte; then `own` (a literal, END_OF_BLOCK at i == N, -1: nothing).
struct Tokens {
    int match, pending, own;
};

// left: the byte before (lane 0: the last trip's last).  carry: the run the last trip ended in, counted from its last
// match of 258.
__device__ __forceinline__ Tokens tokenise(int byte, int left, uint32_t i, uint32_t N, int lane, int &carry)
{
    Tokens t;
    t.match = 0, t.pending = 0, t.own = -1;
    const bool eq = i < N && i > 0 && byte == left;
    const unsigned long long differ = ~__ballot(eq) & ((1ull << lane) - 1); // the lanes below that end a run
    const int last_differ = differ ? 63 - __clzll((long long)differ) : -1;
    int run = 0;
    if (eq) {
        run = differ ? lane - last_differ : carry + lane + 1; // < 258 + 64: it reaches 258 once at the most
        if (run == MAX_MATCH)
            t.match = MAX_MATCH;
    } else if (i <= N) {
        int pending = differ ? lane - 1 - last_differ : carry + lane; // the run that ended at the byte before
        if (pending >= MAX_MATCH)
            pending -= MAX_MATCH; // a lane below has emitted that match
        if (pending >= MIN_MATCH)
            t.match = pending;
        else
            t.pending = pending;
        t.own = i < N ? byte : END_OF_BLOCK;
    }
    carry = __shfl(eq ? (run >= MAX_MATCH ? run - MAX_MATCH : run) : 0, WAVE - 1, WAVE);
    return t;
}

// ---- the frame's own code: count, table -------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_png_count(const uint8_t *__restrict__ filtered, uint32_t row_bytes, int H, int band_rows,
                                                    uint32_t *__restrict__ counts)
{
    __shared__ uint32_t s_cnt[N_SYMBOLS];
    const int lane = threadIdx.x;
    for (int w = lane; w < N_SYMBOLS; w += WAVE)
        s_cnt[w] = 0;
    const int first_row = blockIdx.x * band_rows;
    const int rows = min(band_rows, H - first_row);
    const uint32_t N = (uint32_t)rows * row_bytes;
    const uint8_t *src = filtered + (size_t)first_row * row_bytes;
    int carry = 0, prev_last = 0;
    int cur[TRIPS], next[TRIPS];
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const uint32_t j = (uint32_t)(k * WAVE + lane);
        cur[k] = j < N ? src[j] : 0;
    }
    __syncthreads();
    for (uint32_t block = 0; block <= N; block += TRIPS * WAVE) {
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const uint32_t j = block + (uint32_t)((TRIPS + k) * WAVE + lane);
            next[k] = j < N ? src[j] : 0;
        }
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const uint32_t base = block + (uint32_t)(k * WAVE);
            if (base > N)
                break;
            const int byte = cur[k];
            int left = __shfl_up(byte, 1, WAVE);
            if (lane == 0)
                left = prev_last;
            const Tokens t = tokenise(byte, left, base + lane, N, lane, carry);
            prev_last = __shfl(byte, WAVE - 1, WAVE);
            if (t.match)
                atomicAdd(&s_cnt[257 + length_symbol(t.match)], 1u);
            if (t.pending)
                atomicAdd(&s_cnt[left], (uint32_t)t.pending);
            if (t.own >= 0)
                atomicAdd(&s_cnt[t.own], 1u);
        }
#pragma unroll
        for (int k = 0; k < TRIPS; k++)
            cur[k] = next[k];
    }
    __syncthreads();
    for (int w = lane; w < N_SYMBOLS; w += WAVE) {
        const uint32_t c = s_cnt[w];
        counts[(size_t)blockIdx.x * N_SYMBOLS + w] = c;
    }
}

// The frame's histogram: the column sums of the bands' rows.  64 columns a work-group, a wave per 16th of the rows.
constexpr int TOTAL_BLOCK = 1024;
__global__ __launch_bounds__(TOTAL_BLOCK) void k_png_total(const uint32_t *__restrict__ counts, int n_bands, uint32_t *__restrict__ totals)
{
    __shared__ uint32_t s_sum[TOTAL_BLOCK / WAVE][WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int col = blockIdx.x * WAVE + lane;
    uint32_t sum = 0; // (a frame has less than 2^32 bytes, and a byte brings one token at the most)
    if (col < N_SYMBOLS) {
#pragma unroll 8
        for (int band = wave; band < n_bands; band += TOTAL_BLOCK / WAVE)
            sum += counts[(size_t)band * N_SYMBOLS + col];
    }
    s_sum[wave][lane] = sum;
    __syncthreads();
    if (wave == 0 && col < N_SYMBOLS) {
        sum = 0;
        for (int w = 0; w < TOTAL_BLOCK / WAVE; w++)
            sum += s_sum[w][lane];
        totals[col] = sum;
    }
}

constexpr int HEADER_FIXED_BITS = HEADER_BITS - 4 * (N_SYMBOLS + 1);

__global__ __launch_bounds__(HUFFMAN_BLOCK) void k_png_table(const uint32_t *__restrict__ totals, Tables *__restrict__ out,
                                                             FrameCode *__restrict__ code)
{
    __shared__ HuffmanLds s; // (deflate_code.h)
    __shared__ uint32_t s_header[HEADER_WORDS];
    const int tid = threadIdx.x;
    if (tid < N_SYMBOLS)
        s.w[tid] = totals[tid];
    if (tid < HEADER_WORDS)
        s_header[tid] = 0;
    const uint32_t repairs = huffman_build(s, tid);
    // ---- the entries, in the layout of make_tables
    if (tid <= END_OF_BLOCK)
        out->lit[tid] = ((uint32_t)s.len[tid] << 24) | deflate::reverse_bits(s.code[tid], s.len[tid]);
    if (tid <= MAX_MATCH) {
        uint32_t entry = 0;
        if (tid >= MIN_MATCH) {
            const int k = length_symbol(tid), sym = 257 + k, len = s.len[sym];
            const uint32_t bits = (uint32_t)len + LENGTH_EXTRA[k] + 1; // the code, the extra bits, the distance code 0
            if (len)
                entry = (bits << 24) | deflate::reverse_bits(s.code[sym], len) | ((uint32_t)(tid - LENGTH_BASE[k]) << len);
        }
        out->match[tid] = entry;
    }
    if (tid < N_SYMBOLS) {
        code->cost[tid] = (uint32_t)s.len[tid] + (tid > END_OF_BLOCK ? LENGTH_EXTRA[tid - 257] + 1 : 0);
        code->lengths[tid] = (uint8_t)s.len[tid];
    }
    // ---- the header: the fixed part by one thread, the 4-bit codes of the lengths (the code of a length is the length)
    // one thread each; the last is the distance code's
    if (tid == 0) {
        int n = 0;
        auto put = [&](uint32_t value, int bits) {
            for (int i = 0; i < bits; i++, n++)
                if ((value >> i) & 1)
                    atomicOr(&s_header[n >> 5], 1u << (n & 31));
        };
        put(0, 1), put(2, 2), put(N_SYMBOLS - 257, 5), put(0, 5), put(19 - 4, 4);
        for (int k = 0; k < 19; k++)
            put(CLEN_ORDER[k] >= 16 ? 0 : 4, 3);
        code->repairs = repairs;
    }
    if (tid <= N_SYMBOLS) {
        const int len = tid < N_SYMBOLS ? s.len[tid] : 1;
        const uint32_t v = deflate::reverse_bits((uint32_t)len, 4), at = (uint32_t)(HEADER_FIXED_BITS + 4 * tid);
        if (v) {
            atomicOr(&s_header[at >> 5], v << (at & 31));
            if ((at & 31) > 28)
                atomicOr(&s_header[(at >> 5) + 1], v >> (32 - (at & 31)));
        }
    }
    __syncthreads();
    if (tid < HEADER_WORDS)
        out->header[tid] = s_header[tid];
}

// ---- deflate ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_token(unsigned long long &bits, int &len, uint32_t entry)
{
    bits |= (unsigned long long)(entry & 0xFFFFFFu) << len;
    len += (int)(entry >> 24);
}

__global__ __launch_bounds__(WAVE) void k_png_deflate(const DeflateArgs a)
{
    __shared__ uint32_t s_bits[BIT_WORDS]; // the trip's bits, stream bit 32 w + k in bit k of word w
    __shared__ uint32_t s_lit[END_OF_BLOCK + 1];
    __shared__ uint32_t s_match[MAX_MATCH + 1];
    const int lane = threadIdx.x;
    const int first_row = blockIdx.x * a.band_rows; // (n_bands * band_rows < H + band_rows <= 2^17)
    const int rows = min(a.band_rows, a.H - first_row);
    const uint32_t N = (uint32_t)rows * a.row_bytes; // (at most 2^28: tf_png_create)
    const uint8_t *src = a.filtered + (size_t)first_row * a.row_bytes;
    uint8_t *slot = a.staging + (size_t)blockIdx.x * a.slot_bytes;
    if (a.counts) {
        // ---- the frame's own code: the band's coded bytes from its counts; stored where that is not smaller
        unsigned long long token_bits = 0;
        for (int sym = lane; sym < N_SYMBOLS; sym += WAVE)
            token_bits += (unsigned long long)a.counts[(size_t)blockIdx.x * N_SYMBOLS + sym] * a.code->cost[sym];
        const unsigned long long coded = (HEADER_BITS + wave_sum64(token_bits) + 3 + 7) / 8 + 4;
        const unsigned long long stored = stored_bytes(N);
        if (!(coded < stored)) {
            // blocks of at most 65535 bytes, each behind 00, its length and the length's complement
            for (uint32_t j = lane; j < stored; j += WAVE) {
                const uint32_t blk = j / (STORED_MAX + 5), r = j % (STORED_MAX + 5);
                const uint32_t len = min(STORED_MAX, N - blk * STORED_MAX);
                int v;
                if (r >= 5)
                    v = src[blk * STORED_MAX + (r - 5)];
                else
                    v = r == 0 ? 0 : (int)(((r < 3 ? len : ~len) >> (8 * ((r - 1) & 1))) & 0xFF);
                if (j < a.slot_bytes)
                    slot[j] = (uint8_t)v;
            }
            if (lane == 0) {
                a.lengths[blockIdx.x] = (uint32_t)min(stored, (unsigned long long)a.slot_bytes);
                if (stored > a.slot_bytes)
                    *a.overflow = 1;
            }
            return;
        }
    }
    const Tables &t = *a.tables;
    for (int w = lane; w < BIT_WORDS; w += WAVE)
        s_bits[w] = w < HEADER_WORDS ? t.header[w] : 0;
    for (int w = lane; w <= END_OF_BLOCK; w += WAVE)
        s_lit[w] = t.lit[w];
    for (int w = lane; w <= MAX_MATCH; w += WAVE)
        s_match[w] = t.match[w];
    uint32_t bitpos = HEADER_BITS; // bits in s_bits
    uint32_t outpos = 0;           // bytes in the slot
    int carry = 0;                 // the run the last trip ended in, counted from its last match of 258
    int prev_last = 0;             // the last trip's last byte
    int cur[TRIPS], next[TRIPS]; // a block of TRIPS trips: its bytes are loaded while the block before is coded
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const uint32_t j = (uint32_t)(k * WAVE + lane);
        cur[k] = j < N ? src[j] : 0;
    }
    __syncthreads();
    for (uint32_t block = 0; block <= N; block += TRIPS * WAVE) {
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const uint32_t j = block + (uint32_t)((TRIPS + k) * WAVE + lane);
            next[k] = j < N ? src[j] : 0;
        }
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
        const uint32_t base = block + (uint32_t)(k * WAVE);
        if (base > N)
            break;
        const int byte = cur[k];
        int left = __shfl_up(byte, 1, WAVE);
        if (lane == 0)
            left = prev_last;
        const Tokens tok = tokenise(byte, left, base + lane, N, lane, carry);
        prev_last = __shfl(byte, WAVE - 1, WAVE);
        unsigned long long bits = 0;
        int len = 0;
        if (tok.match)
            put_token(bits, len, s_match[tok.match]);
        for (int k = 0; k < tok.pending; k++)
            put_token(bits, len, s_lit[left]);
        if (tok.own >= 0)
            put_token(bits, len, s_lit[tok.own]);
        len = min(len, LANE_MAX_BITS); // (never: the host checked the table)
        const int incl = wave_inclusive_sum(len, lane);
        if (len) {
            const uint32_t p = bitpos + (uint32_t)(incl - len);
            const uint32_t word = p >> 5, sh = p & 31;
            const uint32_t w0 = (uint32_t)(bits << sh), w1 = (uint32_t)((bits >> 1) >> (31 - sh));
            const uint32_t w2 = (uint32_t)((bits >> 33) >> (31 - sh));
            if (word + 2 < BIT_WORDS) {
                if (w0)
                    atomicOr(&s_bits[word], w0);
                if (w1)
                    atomicOr(&s_bits[word + 1], w1);
                if (w2)
                    atomicOr(&s_bits[word + 2], w2);
            }
        }
        bitpos += (uint32_t)__shfl(incl, WAVE - 1, WAVE);
        // ---- behind end-of-block: three zero bits, zeros to the byte boundary, 00 00 FF FF
        if (base + WAVE > N) {
            bitpos = (bitpos + 3 + 7) & ~7u;
            const uint32_t q = bitpos + 16 + 8 * (uint32_t)lane;
            if (lane < 2 && (q >> 5) < BIT_WORDS)
                atomicOr(&s_bits[q >> 5], 0xFFu << (q & 31));
            bitpos += 32;
        }
        __syncthreads();
        // ---- the trip's whole bytes to the slot
        const uint32_t n_bytes = bitpos >> 3;
        for (uint32_t j = lane; j < n_bytes; j += WAVE)
            if (outpos + j < a.slot_bytes)
                slot[outpos + j] = (uint8_t)(s_bits[j >> 2] >> (8 * (j & 3)));
        outpos += n_bytes;
        // ---- the bits left over go to the front of a zeroed buffer
        const uint32_t rem = bitpos & 7;
        const uint32_t left_over = rem ? (s_bits[n_bytes >> 2] >> (8 * (n_bytes & 3))) & 0xFF : 0;
        const uint32_t used = (bitpos >> 5) + 3;
        __syncthreads();
        for (uint32_t w = lane; w < used && w < BIT_WORDS; w += WAVE)
            s_bits[w] = w == 0 ? left_over : 0;
        bitpos = rem;
        __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < TRIPS; k++)
            cur[k] = next[k];
    }
    if (lane == 0) {
        a.lengths[blockIdx.x] = min(outpos, a.slot_bytes);
        if (outpos > a.slot_bytes)
            *a.overflow = 1;
    }
}

// ---- pack ------------------------------------------------------------------------------------------------------------
constexpr uint32_t IDAT_CRC = 0x35AF061Eu; // crc32("IDAT"); checked against the table when a handle is made

constexpr int PACK_BLOCK = 256;
__global__ __launch_bounds__(PACK_BLOCK) void k_png_pack(const uint8_t *__restrict__ staging, uint32_t slot_bytes,
                                                         const uint32_t *__restrict__ lengths, const uint32_t *__restrict__ offsets, int n,
                                                         const Tables *__restrict__ tables, uint8_t *__restrict__ out, size_t capacity)
{
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_x2n[32];
    s_crc[threadIdx.x] = tables->crc.crc[threadIdx.x]; // (PACK_BLOCK is the table's 256)
    crc32_stage_x2n(s_x2n, &tables->crc, threadIdx.x);
    __syncthreads();
    const int i = blockIdx.x * (PACK_BLOCK / WAVE) + threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (i >= n)
        return;
    const uint8_t *src = staging + (size_t)i * slot_bytes;
    const uint32_t len = min(lengths[i], slot_bytes);
    const size_t dst = (size_t)offsets[i];
    if (lane < 8 && dst + lane < capacity)
        out[dst + lane] = lane < 4 ? (uint8_t)(len >> (24 - 8 * lane)) : (uint8_t)"IDAT"[lane - 4];
    // (slots are dword-aligned and a multiple of four bytes: a dword that holds a byte below len lies inside the slot)
    const uint32_t *src4 = reinterpret_cast<const uint32_t *>(src);
#pragma unroll 4
    for (uint32_t j = 4 * (uint32_t)lane; j < len; j += 4 * WAVE) {
        const uint32_t v = src4[j >> 2];
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
            if (j + b < len && dst + 8 + j + b < capacity)
                out[dst + 8 + j + b] = (uint8_t)(v >> (8 * b));
    }
    // the CRC of "IDAT" and the data: lane l takes bytes [l slice, (l + 1) slice); lane 0 goes on from "IDAT"
    const uint32_t slice = ((len + WAVE - 1) / WAVE + 3) & ~3u; // whole dwords
    const uint32_t begin = min((uint32_t)lane * slice, len), end = min(begin + slice, len);
    uint32_t c = lane == 0 ? ~IDAT_CRC : 0xFFFFFFFFu;
#pragma unroll 4
    for (uint32_t j = begin; j < end; j += 4) {
        const uint32_t v = src4[j >> 2];
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
            if (j + b < end)
                c = crc32_update(c, v >> (8 * b), s_crc);
    }
    c = crc32_wave_xor(crc32_shift(~c, len - end, s_x2n)); // ~c: the slice's own CRC-32 (of no bytes: 0)
    if (lane < 4 && dst + 8 + len + lane < capacity)
        out[dst + 8 + len + lane] = (uint8_t)(c >> (24 - 8 * lane));
}

// ---- host: the code, the tables, the chunks the host writes ------------------------------------------------------------
// The literal/length code: Huffman over model weights, the two smallest merged on the key (weight, order) -- a leaf's
// order is its symbol, the k-th internal node's 1000 + k -- until one is left; a symbol's length is its leaf's depth.
static void make_code_lengths(uint8_t lengths[N_SYMBOLS])
{
    struct Node {
        uint64_t weight;
        int order, parent;
        bool live;
    };
    std::vector<Node> nodes;
    for (int v = 0; v < 256; v++) {
        const uint64_t m = (uint64_t)(v < 256 - v ? v : 256 - v) + 1, cube = m * m * m;
        uint64_t root = 0;
        while ((root + 1) * (root + 1) <= cube)
            root++;
        const uint64_t w = 65536 / root;
        nodes.push_back({w < 128 ? 128 : w, v, -1, true});
    }
    nodes.push_back({128, END_OF_BLOCK, -1, true});
    for (int k = 0; k < N_LENGTH_SYMBOLS; k++)
        nodes.push_back({k == N_LENGTH_SYMBOLS - 1 ? 4096u : 512u, 257 + k, -1, true});
    for (int k = 0;; k++) {
        int lo[2] = {-1, -1};
        for (int pick = 0; pick < 2; pick++)
            for (int i = 0; i < (int)nodes.size(); i++) {
                if (!nodes[i].live || i == lo[0])
                    continue;
                const int j = lo[pick];
                if (j < 0 || nodes[i].weight < nodes[j].weight || (nodes[i].weight == nodes[j].weight && nodes[i].order < nodes[j].order))
                    lo[pick] = i;
            }
        if (lo[1] < 0)
            break;
        nodes[lo[0]].live = nodes[lo[1]].live = false;
        nodes[lo[0]].parent = nodes[lo[1]].parent = (int)nodes.size();
        nodes.push_back({nodes[lo[0]].weight + nodes[lo[1]].weight, 1000 + k, -1, true});
    }
    for (int s = 0; s < N_SYMBOLS; s++) {
        int depth = 0;
        for (int i = s; nodes[i].parent >= 0; i = nodes[i].parent)
            depth++;
        lengths[s] = (uint8_t)(depth > 255 ? 255 : depth);
    }
}

static uint32_t reverse_bits(uint32_t code, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; i++)
        r |= ((code >> i) & 1) << (n - 1 - i);
    return r;
}

struct HeaderBits {
    uint32_t words[HEADER_WORDS] = {};
    int n = 0;
    void put(uint32_t value, int bits)
    {
        for (int i = 0; i < bits; i++, n++)
            if ((value >> i) & 1)
                words[n >> 5] |= 1u << (n & 31);
    }
};

// Everything the kernels read; byte_bits and eob_bits for the bound.  TF_ERR_STATE if the code is not what the kernels
// are written for (complete, at most 15 bits, a lane's tokens within 64).
static int make_tables(Tables &t, int *byte_bits, int *eob_bits)
{
    uint8_t len[N_SYMBOLS];
    make_code_lengths(len);
    // RFC 1951 3.2.2
    int count[17] = {}, longest = 0;
    uint64_t kraft = 0; // in units of 2^-16
    for (int s = 0; s < N_SYMBOLS; s++) {
        if (len[s] < 1 || len[s] > 15)
            return set_error(TF_ERR_STATE, "png: symbol %d has a code of %d bits", s, len[s]);
        count[len[s]]++, kraft += 1ull << (16 - len[s]);
        longest = len[s] > longest ? len[s] : longest;
    }
    if (kraft != 1ull << 16)
        return set_error(TF_ERR_STATE, "png: the literal/length code is not complete");
    uint32_t next_code[17] = {}, code = 0, codes[N_SYMBOLS];
    for (int bits = 1; bits <= 15; bits++) {
        code = (code + count[bits - 1]) << 1;
        next_code[bits] = code;
    }
    for (int s = 0; s < N_SYMBOLS; s++)
        codes[s] = next_code[len[s]]++;
    int worst = 0, longest_lit = 0, longest_match = 0;
    for (int s = 0; s <= END_OF_BLOCK; s++) {
        t.lit[s] = ((uint32_t)len[s] << 24) | reverse_bits(codes[s], len[s]);
        if (s < END_OF_BLOCK)
            longest_lit = len[s] > longest_lit ? len[s] : longest_lit;
    }
    worst = longest_lit;
    for (int n = 0; n <= MAX_MATCH; n++)
        t.match[n] = 0;
    for (int k = 0; k < N_LENGTH_SYMBOLS; k++) {
        const int s = 257 + k, last = k + 1 < N_LENGTH_SYMBOLS ? LENGTH_BASE[k + 1] - 1 : MAX_MATCH;
        for (int n = LENGTH_BASE[k]; n <= last && (k == N_LENGTH_SYMBOLS - 1 || n < MAX_MATCH); n++) {
            const int bits = len[s] + LENGTH_EXTRA[k] + 1; // the code, the extra bits, the distance code 0
            t.match[n] = ((uint32_t)bits << 24) | reverse_bits(codes[s], len[s]) | ((uint32_t)(n - LENGTH_BASE[k]) << len[s]);
            const int per_byte = (bits + n - 1) / n;
            worst = per_byte > worst ? per_byte : worst;
            longest_match = bits > longest_match ? bits : longest_match;
        }
    }
    // a lane's tokens: a match or two literals, then its own literal or end-of-block
    const int own = longest_lit > len[END_OF_BLOCK] ? longest_lit : len[END_OF_BLOCK];
    if (2 * longest_lit + own > LANE_MAX_BITS || longest_match + own > LANE_MAX_BITS || longest_match > 24)
        return set_error(TF_ERR_STATE, "png: a lane's tokens would not fit %d bits", LANE_MAX_BITS);
    *byte_bits = worst, *eob_bits = len[END_OF_BLOCK];

    make_crc32_consts(t.crc);

    HeaderBits h;
    h.put(0, 1), h.put(2, 2), h.put(N_SYMBOLS - 257, 5), h.put(0, 5), h.put(19 - 4, 4);
    for (int k = 0; k < 19; k++)
        h.put(CLEN_ORDER[k] >= 16 ? 0 : 4, 3);
    for (int s = 0; s <= N_SYMBOLS; s++) // the lengths' 4-bit codes are the lengths; the last is the distance code's
        h.put(reverse_bits(s < N_SYMBOLS ? len[s] : 1, 4), 4);
    if (h.n != HEADER_BITS)
        return set_error(TF_ERR_STATE, "png: the table header has %d bits, not %d", h.n, HEADER_BITS);
    memcpy(t.header, h.words, sizeof(t.header));
    return TF_OK;
}

static void put_be32(std::vector<uint8_t> &out, uint32_t v)
{
    for (int k = 0; k < 4; k++)
        out.push_back((uint8_t)(v >> (24 - 8 * k)));
}

static void put_chunk(std::vector<uint8_t> &out, const Tables &t, const char *kind, const std::vector<uint8_t> &payload)
{
    put_be32(out, (uint32_t)payload.size());
    const size_t at = out.size();
    out.insert(out.end(), kind, kind + 4);
    out.insert(out.end(), payload.begin(), payload.end());
    put_be32(out, crc32_bytes(t.crc, out.data() + at, out.size() - at));
}

static int default_band_rows(int height, int width)
{
    const long row = 3L * width + 1;
    const long rows = (DEFAULT_BAND_BYTES + row - 1) / row;
    return (int)(rows < 1 ? 1 : (rows > height ? height : rows));
}

} // namespace png
} // namespace tf

using namespace tf;
using namespace tf::png;

struct tf_png {
    int H = 0, W = 0, band_rows = 0, n_bands = 0;
    uint32_t row_bytes = 0;
    Tables tables;
    std::vector<uint8_t> head, tail; // what the host writes in front of the bands' chunks and behind them
    DevBuf dev_tables, filtered, rowsums, upload;
    SlotStream s; // a slot a band; packed, the bands' IDAT chunks
    // the frame's own code (tf_png_set_code): allocated by the first encode that uses it
    int code = 0;
    DevBuf counts, totals, frame_tables, frame_code;
    PinnedBuf frame_code_host; // page-locked FrameCode: the last frame's
    PinnedBuf lengths_host;    // page-locked uint32_t: the last frame's bands' bytes
    bool last_own_code = false; // the last encode that ran used the frame's own code: the two buffers above hold it
    PinnedBuf rowsums_host; // page-locked uint32_t: the rows' Adler sums
};

// What the host writes in front of the bands' chunks: the signature, IHDR, with `index` the band index tfBX (version 1,
// flags 0, 0, band_rows, n_bands), and the IDAT of the zlib header.
static void make_head(tf_png *enc, bool index)
{
    enc->head = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, (uint32_t)enc->W), put_be32(ihdr, (uint32_t)enc->H);
    ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});
    put_chunk(enc->head, enc->tables, "IHDR", ihdr);
    if (index) {
        std::vector<uint8_t> bands{1, 0, 0, 0};
        put_be32(bands, (uint32_t)enc->band_rows), put_be32(bands, (uint32_t)enc->n_bands);
        put_chunk(enc->head, enc->tables, "tfBX", bands);
    }
    put_chunk(enc->head, enc->tables, "IDAT", {0x78, 0x01});
}

TF_API int tf_png_set_index(tf_png *enc, int on)
{
    TF_REQUIRE(enc, "tf_png_set_index: null pointer");
    make_head(enc, on != 0);
    enc->s.last = 0; // the head of the last encode is gone: nothing to copy again
    return TF_OK;
}

TF_API int tf_png_set_code(tf_png *enc, int mode)
{
    TF_REQUIRE(enc, "tf_png_set_code: null pointer");
    TF_REQUIRE(mode == 0 || mode == 1, "tf_png_set_code: mode %d (0: the library's code, 1: the frame's own)", mode);
    if (mode == 1) {
        // whatever code a histogram gives: a lane's tokens of a trip -- three literals, or a match and a literal -- fit
        // its 64-bit accumulator, a match its entry's 24 bits, and a band's stored form its slot
        constexpr int MATCH_BITS = MAX_CODE_BITS + 5 + 1;
        static_assert(3 * MAX_CODE_BITS <= LANE_MAX_BITS && MATCH_BITS + MAX_CODE_BITS <= LANE_MAX_BITS, "a lane's tokens outgrow its accumulator");
        static_assert(MATCH_BITS <= 24, "a match outgrows its entry");
        const uint64_t band = (uint64_t)enc->band_rows * enc->row_bytes;
        if (stored_bytes(band) > enc->s.slot)
            return set_error(TF_ERR_STATE, "tf_png_set_code: a stored band of %llu bytes would not fit its slot of %u",
                             (unsigned long long)stored_bytes(band), enc->s.slot);
    }
    enc->code = mode;
    return TF_OK;
}

TF_API void tf_png_destroy(tf_png *enc) { delete enc; }

TF_API int tf_png_default_band_rows(int height, int width)
{
    if (height < 1 || width < 1)
        return 0;
    return default_band_rows(height, width);
}

TF_API int tf_png_code_lengths(uint8_t *out)
{
    TF_REQUIRE(out, "tf_png_code_lengths: null pointer");
    make_code_lengths(out);
    return TF_OK;
}

TF_API int tf_png_create(tf_png **out, int height, int width, int band_rows)
{
    TF_REQUIRE(out, "tf_png_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(height >= 1 && width >= 1 && height <= 65535 && width <= 65535, "tf_png_create: bad size %dx%d (1 to 65535)", width,
               height);
    TF_REQUIRE(band_rows >= 0, "tf_png_create: band_rows %d (0 = default, 1 or more)", band_rows);
    const int rows = band_rows == 0 ? default_band_rows(height, width) : (band_rows > height ? height : band_rows);
    const size_t row_bytes = 3 * (size_t)width + 1;
    TF_REQUIRE(rows * row_bytes <= (size_t)1 << 28, "tf_png_create: a band of %d rows has %zu bytes (at most 2^28)", rows,
               rows * row_bytes);
    TF_TRY(ensure_init());
    auto enc = make_handle<tf_png>();
    TF_REQUIRE(enc, "tf_png_create: out of memory");
    enc->H = height, enc->W = width, enc->band_rows = rows, enc->row_bytes = (uint32_t)row_bytes;
    enc->n_bands = (height + rows - 1) / rows;
    int byte_bits = 0, eob_bits = 0;
    TF_TRY(make_tables(enc->tables, &byte_bits, &eob_bits));
    const size_t n = (size_t)enc->n_bands, slot = slot_bytes(rows * row_bytes, byte_bits, eob_bits);
    // offsets are 32-bit
    TF_REQUIRE(n * (slot + 12) < (size_t)1 << 32, "tf_png_create: %dx%d in bands of %d rows could take %zu bytes (less than 2^32)", width,
               height, rows, n * (slot + 12));
    if (crc32_bytes(enc->tables.crc, (const uint8_t *)"IDAT", 4) != IDAT_CRC)
        return set_error(TF_ERR_STATE, "tf_png_create: the CRC table is wrong");
    make_head(enc.get(), false);
    TF_TRY(enc->dev_tables.alloc(sizeof(Tables)));
    TF_TRY(enc->filtered.alloc((size_t)height * row_bytes));
    TF_TRY(enc->rowsums.alloc((size_t)height * 2 * sizeof(uint32_t)));
    TF_TRY(enc->s.alloc(enc->n_bands, (uint32_t)slot, 12)); // a chunk: length, type, data, CRC
    TF_TRY(enc->rowsums_host.alloc(enc->rowsums.bytes));
    TF_HIP(hipMemcpyAsync(enc->dev_tables.p, &enc->tables, sizeof(Tables), hipMemcpyHostToDevice, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    *out = enc.release();
    return TF_OK;
}

TF_API int tf_png_band_rows(tf_png *enc)
{
    return enc ? enc->band_rows : 0;
}

// what the frame's own code takes beside the handle's other buffers
static int own_code_buffers(tf_png *enc)
{
    if (enc->lengths_host.p)
        return TF_OK;
    TF_TRY(enc->counts.alloc((size_t)enc->n_bands * N_SYMBOLS * sizeof(uint32_t)));
    TF_TRY(enc->totals.alloc(N_SYMBOLS * sizeof(uint32_t)));
    TF_TRY(enc->frame_tables.alloc(sizeof(Tables)));
    TF_TRY(enc->frame_code.alloc(sizeof(FrameCode)));
    TF_TRY(enc->frame_code_host.alloc(sizeof(FrameCode)));
    return enc->lengths_host.alloc(enc->s.lengths.bytes);
}

// the slots to their chunks in the packed stream, as far as the caller's `capacity` reaches behind the head
static int pack(tf_png *enc, size_t capacity)
{
    const SlotStream &s = enc->s;
    return launch("png_pack", k_png_pack, dim3(cdiv(s.n, PACK_BLOCK / WAVE)), dim3(PACK_BLOCK), 0, s.staging.as<uint8_t>(), s.slot,
                  s.lengths.as<uint32_t>(), s.offsets.as<uint32_t>(), s.n, enc->dev_tables.as<Tables>(), s.packed.as<uint8_t>(),
                  s.pack_room(capacity, enc->head.size()));
}

TF_API int tf_png_encode_dev(tf_png *enc, const void *rgb_dev, uint8_t *out, size_t capacity, size_t *n_bytes)
{
    TF_REQUIRE(enc && rgb_dev && n_bytes && (out || capacity == 0), "tf_png_encode_dev: null pointer");
    *n_bytes = 0;
    SlotStream &s = enc->s;
    TF_TRY(s.begin());
    TF_TRY(launch("png_filter", k_png_filter, dim3(enc->H), dim3(FILTER_BLOCK), 0, (const uint8_t *)rgb_dev, enc->W,
                  enc->filtered.as<uint8_t>(), enc->rowsums.as<uint32_t>()));
    DeflateArgs a;
    a.filtered = enc->filtered.as<uint8_t>(), a.row_bytes = enc->row_bytes, a.H = enc->H, a.band_rows = enc->band_rows;
    a.tables = enc->dev_tables.as<Tables>(), a.counts = nullptr, a.code = nullptr;
    a.staging = s.staging.as<uint8_t>(), a.slot_bytes = s.slot;
    enc->last_own_code = false;
    if (enc->code) {
        TF_TRY(own_code_buffers(enc));
        TF_TRY(launch("png_count", k_png_count, dim3(enc->n_bands), dim3(WAVE), 0, a.filtered, a.row_bytes, a.H, a.band_rows,
                      enc->counts.as<uint32_t>()));
        TF_TRY(launch("png_total", k_png_total, dim3(cdiv(N_SYMBOLS, WAVE)), dim3(TOTAL_BLOCK), 0, enc->counts.as<uint32_t>(), enc->n_bands,
                      enc->totals.as<uint32_t>()));
        TF_TRY(launch("png_table", k_png_table, dim3(1), dim3(HUFFMAN_BLOCK), 0, enc->totals.as<uint32_t>(), enc->frame_tables.as<Tables>(),
                      enc->frame_code.as<FrameCode>()));
        a.tables = enc->frame_tables.as<Tables>(), a.counts = enc->counts.as<uint32_t>(), a.code = enc->frame_code.as<FrameCode>();
    }
    a.lengths = s.lengths.as<uint32_t>();
    a.overflow = s.overflow();
    TF_TRY(launch("png_deflate", k_png_deflate, dim3(enc->n_bands), dim3(WAVE), 0, a));
    TF_TRY(s.scan("png_scan"));
    TF_TRY(pack(enc, capacity));
    TF_TRY(s.fetch());
    TF_HIP(hipMemcpyAsync(enc->rowsums_host.p, enc->rowsums.p, enc->rowsums.bytes, hipMemcpyDeviceToHost, stream()));
    if (enc->code) {
        TF_HIP(hipMemcpyAsync(enc->frame_code_host.p, enc->frame_code.p, sizeof(FrameCode), hipMemcpyDeviceToHost, stream()));
        TF_HIP(hipMemcpyAsync(enc->lengths_host.p, s.lengths.p, s.lengths.bytes, hipMemcpyDeviceToHost, stream()));
    }
    TF_HIP(hipStreamSynchronize(stream()));
    TF_TRY(s.finish("tf_png_encode_dev", "a band"));
    // Adler-32 of the whole stream from the rows' sums: a row of L bytes moves s2 by L s1 + its weighted sum
    uint64_t s1 = 1, s2 = 0;
    for (int r = 0; r < enc->H; r++) {
        s2 = (s2 + (enc->row_bytes % ADLER_BASE) * s1 + enc->rowsums_host.as<uint32_t>()[2 * r + 1]) % ADLER_BASE;
        s1 = (s1 + enc->rowsums_host.as<uint32_t>()[2 * r]) % ADLER_BASE;
    }
    enc->tail.clear();
    std::vector<uint8_t> last{0x01, 0x00, 0x00, 0xFF, 0xFF};
    put_be32(last, (uint32_t)((s2 << 16) | s1));
    put_chunk(enc->tail, enc->tables, "IDAT", last);
    put_chunk(enc->tail, enc->tables, "IEND", {});
    enc->last_own_code = enc->code != 0;
    return s.copy_out("tf_png_encode_dev", enc->head, enc->tail, out, capacity, n_bytes);
}

TF_API int tf_png_last_code(tf_png *enc, uint8_t *lengths, uint32_t *repairs)
{
    TF_REQUIRE(enc && lengths && repairs, "tf_png_last_code: null pointer");
    if (!enc->last_own_code)
        return set_error(TF_ERR_STATE, "tf_png_last_code: no frame has been encoded with its own code");
    const FrameCode *code = enc->frame_code_host.as<FrameCode>();
    memcpy(lengths, code->lengths, N_SYMBOLS);
    *repairs = code->repairs;
    return TF_OK;
}

TF_API int tf_png_last_bands(tf_png *enc, uint32_t *sizes, uint8_t *stored, size_t capacity, size_t *n_bands)
{
    TF_REQUIRE(enc && n_bands && ((sizes && stored) || capacity == 0), "tf_png_last_bands: null pointer");
    *n_bands = 0;
    if (!enc->last_own_code)
        return set_error(TF_ERR_STATE, "tf_png_last_bands: no frame has been encoded with its own code");
    *n_bands = (size_t)enc->n_bands;
    TF_REQUIRE(*n_bands <= capacity, "tf_png_last_bands: %zu bands, room for %zu", *n_bands, capacity);
    for (int i = 0; i < enc->n_bands; i++) {
        // a band is coded only where that is smaller than its stored form: the size says which it is
        const int rows = enc->band_rows < enc->H - i * enc->band_rows ? enc->band_rows : enc->H - i * enc->band_rows;
        sizes[i] = enc->lengths_host.as<uint32_t>()[i];
        stored[i] = sizes[i] == stored_bytes((uint64_t)rows * enc->row_bytes);
    }
    return TF_OK;
}

TF_API int tf_png_copy_last(tf_png *enc, uint8_t *out, size_t capacity, size_t *n_bytes)
{
    TF_REQUIRE(enc && n_bytes && (out || capacity == 0), "tf_png_copy_last: null pointer");
    *n_bytes = 0;
    TF_TRY(enc->s.have_last("tf_png_copy_last"));
    TF_TRY(pack(enc, capacity));
    return enc->s.copy_out("tf_png_copy_last", enc->head, enc->tail, out, capacity, n_bytes);
}

TF_API int tf_png_encode(tf_png *enc, const uint8_t *rgb_host, uint8_t *out, size_t capacity, size_t *n_bytes)
{
    TF_REQUIRE(enc && rgb_host && n_bytes, "tf_png_encode: null pointer");
    const size_t bytes = (size_t)enc->H * enc->W * 3;
    TF_TRY(enc->upload.upload(rgb_host, bytes));
    return tf_png_encode_dev(enc, enc->upload.p, out, capacity, n_bytes);
}
