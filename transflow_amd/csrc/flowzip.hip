// A flow archive member -- the `.npy` header and the array's bytes, S = prefix ‖ data -- as the raw deflate stream a zip
// holds, made where the array is (tests/flowzip_ref.py is the numpy statement of the same rules).
//
// S is cut into bands of `band_bytes` that are coded side by side.  A band is one dynamic-Huffman block and an empty
// stored block that brings it to a byte boundary, or, where that would not be smaller, stored blocks.  Matches are
// "the same byte D back" stretches, never across the band's first byte.  The literal/length code is the member's own:
//
//   k_fz_count   one wave per band, 64 bytes a trip.  A lane compares its byte with the one D lanes back (the first D
//                lanes with the last D bytes of the trip before); the ballot of equal lanes and the count carried from
//                the trip before give it its place in a stretch, as in k_png_deflate.  The tokens are counted: the band's
//                286 counts go to its row and, by integer atomics, to the member's histogram.  Then the band's CRC-32:
//                the lanes take contiguous slices, the slices' CRCs are combined by x^(8 * bytes behind).
//   k_fz_table   one work-group.  The code of the histogram (deflate_code.h: the used symbols ranked by (weight, symbol),
//                the two smallest merged on the key (weight, order), weights halved and the code rebuilt while a length
//                exceeds 15, canonical codes), then the token entries and the header bits.
//   k_fz_sizes   one wave per band: its coded bits from its counts and the code, coded or stored, its bytes.
//   k_fz_scan    exclusive sum of the bands' bytes (one work-group, chunks of 1024 bands), the member's CRC-32 from the
//                bands', and the final block 01 00 00 FF FF behind the last band.
//   k_fz_emit    one wave per band.  The same tokeniser; a wave prefix sum of the bit counts places the tokens in an
//                LDS bit buffer that starts out holding the header; after every trip its whole bytes go straight to
//                the band's place in the stream.  A stored band is copied behind its block headers.  Every store is
//                checked against the buffer's capacity.
//   k_fz_round   numpy.round(flow).astype(int): half to even in the input's type, int64 out.
#include "flowzip_common.h"
#include "stream_common.h"

#include <cstring>

namespace tf {
namespace flowzip {

struct Stream {
    const uint8_t *prefix; // prefix_len bytes, a multiple of 64
    const uint8_t *data;
    uint32_t prefix_len;
    uint32_t N;            // prefix_len + the data's bytes
    uint32_t band_bytes;   // a multiple of 64
    int distance;
};

// byte i of S (i < N)
__device__ __forceinline__ int stream_byte(const Stream &s, uint32_t i)
{
    return i < s.prefix_len ? s.prefix[i] : s.data[i - s.prefix_len];
}

// ---- the tokeniser -----------------------------------------------------------------------------------------------------
// What the lane of band byte i emits in a trip, in stream order: a match of `match` bytes, or `pending` (0 - 2) literals
// `older`, `newer`; then `own` (a literal, END_OF_BLOCK at i == n, -1: nothing).
struct Tokens {
    int match, pending, older, newer, own;
};

// the value `d` lanes back (1 <= d <= 64): this trip's below lane d, the trip before's in the lanes under it
__device__ __forceinline__ int lanes_back(int cur, int prev, int d, int lane)
{
    const int from = (lane - d) & (WAVE - 1);
    const int a = __shfl(cur, from, WAVE), b = __shfl(prev, from, WAVE);
    return lane >= d ? a : b;
}

// carry: the stretch the last trip ended in, counted from its last match of 258
__device__ __forceinline__ Tokens tokenise(int byte, int prev, uint32_t i, uint32_t n, int D, int lane, int &carry)
{
    Tokens t;
    const int back = lanes_back(byte, prev, D, lane);
    t.newer = lanes_back(byte, prev, 1, lane);
    t.older = lanes_back(byte, prev, 2, lane);
    t.match = 0, t.pending = 0, t.own = -1;
    const bool eq = i < n && i >= (uint32_t)D && byte == back;
    const unsigned long long differ = ~__ballot(eq) & ((1ull << lane) - 1); // the lanes below that end a stretch
    const int last_differ = differ ? 63 - __clzll((long long)differ) : -1;
    int run = 0;
    if (eq) {
        run = differ ? lane - last_differ : carry + lane + 1; // < 258 + 64: it reaches 258 once at the most
        if (run == MAX_MATCH)
            t.match = MAX_MATCH;
    } else if (i <= n) {
        int pending = differ ? lane - 1 - last_differ : carry + lane; // the stretch that ended at the byte before
        if (pending >= MAX_MATCH)
            pending -= MAX_MATCH; // a lane below has emitted that match
        if (pending >= MIN_MATCH)
            t.match = pending;
        else
            t.pending = pending;
        t.own = i < n ? byte : END_OF_BLOCK;
    }
    carry = __shfl(eq ? (run >= MAX_MATCH ? run - MAX_MATCH : run) : 0, WAVE - 1, WAVE);
    return t;
}

constexpr int TRIPS = 4; // a block of trips: its bytes are loaded while the block before is coded

// ---- count -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_fz_count(const Stream s, const Crc32Consts *__restrict__ consts, uint32_t *__restrict__ counts,
                                                   uint32_t *__restrict__ totals, uint32_t *__restrict__ band_crc)
{
    __shared__ uint32_t s_cnt[N_SYMBOLS];
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_x2n[32];
    const int lane = threadIdx.x;
    for (int w = lane; w < N_SYMBOLS; w += WAVE)
        s_cnt[w] = 0;
    for (int w = lane; w < 256; w += WAVE)
        s_crc[w] = consts->crc[w];
    if (lane < 32)
        s_x2n[lane] = consts->x2n[lane];
    const uint32_t first = blockIdx.x * s.band_bytes; // (n_bands * band_bytes < N + band_bytes < 2^32: tf_flowzip_create)
    const uint32_t n = min(s.band_bytes, s.N - first);
    int carry = 0, prev = 0;
    int cur[TRIPS], next[TRIPS];
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const uint32_t j = (uint32_t)(k * WAVE + lane);
        cur[k] = j < n ? stream_byte(s, first + j) : 0;
    }
    __syncthreads();
    for (uint32_t block = 0; block <= n; block += TRIPS * WAVE) {
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const uint32_t j = block + (uint32_t)((TRIPS + k) * WAVE + lane);
            next[k] = j < n ? stream_byte(s, first + j) : 0;
        }
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const uint32_t base = block + (uint32_t)(k * WAVE);
            if (base > n)
                break;
            const Tokens t = tokenise(cur[k], prev, base + lane, n, s.distance, lane, carry);
            prev = cur[k];
            if (t.match)
                atomicAdd(&s_cnt[257 + length_symbol(t.match)], 1u);
            if (t.pending == 2)
                atomicAdd(&s_cnt[t.older], 1u);
            if (t.pending >= 1)
                atomicAdd(&s_cnt[t.newer], 1u);
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
        if (c)
            atomicAdd(&totals[w], c);
    }
    // the band's CRC-32: lane l takes bytes [l slice, (l + 1) slice)
    const uint32_t slice = (n + WAVE - 1) / WAVE;
    const uint32_t begin = min((uint32_t)lane * slice, n), end = min(begin + slice, n);
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t j = begin; j < end; j++)
        c = s_crc[(c ^ (uint32_t)stream_byte(s, first + j)) & 0xFF] ^ (c >> 8);
    c = ~c; // the slice's own CRC-32 (of no bytes: 0)
    if (c && end < n)
        c = multmodp(x8nmodp(n - end, s_x2n), c);
#pragma unroll
    for (int d = WAVE / 2; d; d >>= 1)
        c ^= __shfl_xor(c, d, WAVE);
    if (lane == 0)
        band_crc[blockIdx.x] = c;
}

// ---- table -------------------------------------------------------------------------------------------------------------
constexpr int TABLE_BLOCK = HUFFMAN_BLOCK;

__global__ __launch_bounds__(TABLE_BLOCK) void k_fz_table(const uint32_t *__restrict__ totals, int distance, Tables *__restrict__ out)
{
    __shared__ HuffmanLds s; // (deflate_code.h)
    __shared__ uint32_t s_header[HEADER_WORDS];
    const int tid = threadIdx.x;
    if (tid < N_SYMBOLS)
        s.w[tid] = totals[tid];
    if (tid < HEADER_WORDS)
        s_header[tid] = 0;
    const uint32_t repairs = huffman_build(s, tid);
    const int *s_len = s.len;
    const uint32_t *s_code = s.code;
    // ---- the distance symbol that contains `distance`
    int hdist = 0;
    while (hdist + 1 < N_DIST_SYMBOLS && DIST_BASE[hdist + 1] <= distance)
        hdist++;
    const uint32_t dist_value = (uint32_t)(distance - DIST_BASE[hdist]), dist_bits = DIST_EXTRA[hdist];
    // ---- the entries
    if (tid <= END_OF_BLOCK)
        out->lit[tid] = ((uint32_t)s_len[tid] << ENTRY_SHIFT) | reverse_bits(s_code[tid], s_len[tid]);
    if (tid <= MAX_MATCH) {
        uint32_t entry = 0;
        if (tid >= MIN_MATCH) {
            const int k = length_symbol(tid), sym = 257 + k, len = s_len[sym];
            const uint32_t bits = (uint32_t)len + LENGTH_EXTRA[k] + 1 + dist_bits;
            entry = (bits << ENTRY_SHIFT) | reverse_bits(s_code[sym], len) | ((uint32_t)(tid - LENGTH_BASE[k]) << len) |
                    (dist_value << (len + LENGTH_EXTRA[k] + 1));
        }
        out->match[tid] = entry;
    }
    if (tid < N_SYMBOLS) {
        out->cost[tid] = (uint32_t)s_len[tid] + (tid > END_OF_BLOCK ? LENGTH_EXTRA[tid - 257] + 1 + dist_bits : 0);
        out->lengths[tid] = (uint8_t)s_len[tid];
    }
    // ---- the header: the fixed part by one thread, the 4-bit codes of the lengths (the code of a length is the length)
    // one thread each
    if (tid == 0) {
        int n = 0;
        auto put = [&](uint32_t value, int bits) {
            for (int i = 0; i < bits; i++, n++)
                if ((value >> i) & 1)
                    atomicOr(&s_header[n >> 5], 1u << (n & 31));
        };
        put(0, 1), put(2, 2), put(N_SYMBOLS - 257, 5), put((uint32_t)hdist, 5), put(19 - 4, 4);
        for (int k = 0; k < 19; k++)
            put(CLEN_ORDER[k] >= 16 ? 0 : 4, 3);
        out->header_bits = (uint32_t)(HEADER_FIXED_BITS + 4 * (N_SYMBOLS + hdist + 1));
        out->repairs = repairs;
    }
    if (tid < N_SYMBOLS + hdist + 1) {
        const int len = tid < N_SYMBOLS ? s_len[tid] : (tid == N_SYMBOLS + hdist ? 1 : 0);
        const uint32_t v = reverse_bits((uint32_t)len, 4), at = (uint32_t)(HEADER_FIXED_BITS + 4 * tid);
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

// ---- sizes -------------------------------------------------------------------------------------------------------------
constexpr int SIZES_BLOCK = 256;
__global__ __launch_bounds__(SIZES_BLOCK) void k_fz_sizes(const uint32_t *__restrict__ counts, const Tables *__restrict__ tables,
                                                          uint32_t N, uint32_t band_bytes, int n_bands, uint32_t *__restrict__ sizes)
{
    const int band = blockIdx.x * (SIZES_BLOCK / WAVE) + threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (band >= n_bands)
        return;
    unsigned long long bits = 0;
    for (int sym = lane; sym < N_SYMBOLS; sym += WAVE)
        bits += (unsigned long long)counts[(size_t)band * N_SYMBOLS + sym] * tables->cost[sym];
#pragma unroll
    for (int d = WAVE / 2; d; d >>= 1)
        bits += __shfl_xor(bits, d, WAVE);
    bits += tables->header_bits;
    const unsigned long long coded = (bits + 3 + 7) / 8 + 4;
    const uint32_t n = min(band_bytes, N - (uint32_t)band * band_bytes);
    const unsigned long long stored = stored_bytes(n);
    if (lane == 0)
        sizes[band] = coded < stored ? (uint32_t)coded | CODED_FLAG : (uint32_t)stored;
}

// ---- scan: sizes[n] -> offsets[n], exclusive; info[0] = the stream's bytes, info[2] = the member's CRC-32 --------------
__global__ __launch_bounds__(SCAN_BLOCK) void k_fz_scan(const uint32_t *__restrict__ sizes, unsigned long long *__restrict__ offsets, int n,
                                                        const uint32_t *__restrict__ band_crc, const Crc32Consts *__restrict__ consts, uint32_t N,
                                                        uint32_t band_bytes, uint8_t *__restrict__ out, size_t capacity,
                                                        unsigned long long *__restrict__ info)
{
    __shared__ unsigned long long s_wave[SCAN_BLOCK / WAVE];
    __shared__ unsigned long long s_carry;
    __shared__ uint32_t s_x2n[32];
    __shared__ uint32_t s_crc;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    if (tid == 0)
        s_carry = 0, s_crc = 0;
    crc32_stage_x2n(s_x2n, consts, tid);
    __syncthreads();
    uint32_t crc = 0;
    for (int base = 0; base < n; base += SCAN_BLOCK) {
        const int i = base + tid;
        const unsigned long long v = i < n ? (unsigned long long)(sizes[i] & ~CODED_FLAG) : 0;
        const unsigned long long incl = wave_inclusive_sum(v, lane);
        if (lane == WAVE - 1)
            s_wave[wave] = incl;
        __syncthreads();
        unsigned long long before = s_carry;
        for (int w = 0; w < wave; w++)
            before += s_wave[w];
        if (i < n) {
            offsets[i] = before + incl - v;
            // the band's CRC moved in front of the bytes behind it
            const unsigned long long end = min((unsigned long long)N, ((unsigned long long)i + 1) * band_bytes);
            crc ^= crc32_shift(band_crc[i], N - (uint32_t)end, s_x2n);
        }
        __syncthreads();
        if (tid == SCAN_BLOCK - 1)
            s_carry = before + incl;
        __syncthreads();
    }
    crc = crc32_wave_xor(crc);
    if (lane == 0 && crc)
        atomicXor(&s_crc, crc);
    __syncthreads();
    const unsigned long long total = s_carry;
    if (tid < 5) { // the final block: stored, empty
        if (total + tid < capacity)
            out[total + tid] = tid == 0 ? 0x01 : (tid < 3 ? 0x00 : 0xFF);
        else
            info[1] = 1;
    }
    if (tid == 0)
        info[0] = total + 5, info[2] = s_crc;
}

// ---- emit ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_token(unsigned long long &bits, int &len, uint32_t entry)
{
    bits |= (unsigned long long)(entry & ENTRY_MASK) << len;
    len += (int)(entry >> ENTRY_SHIFT);
}

__global__ __launch_bounds__(WAVE) void k_fz_emit(const Stream s, const Tables *__restrict__ tables, const uint32_t *__restrict__ sizes,
                                                  const unsigned long long *__restrict__ offsets, uint8_t *__restrict__ out,
                                                  size_t capacity, unsigned long long *__restrict__ info)
{
    __shared__ uint32_t s_bits[BIT_WORDS]; // the trip's bits, stream bit 32 w + k in bit k of word w
    __shared__ uint32_t s_lit[END_OF_BLOCK + 1];
    __shared__ uint32_t s_match[MAX_MATCH + 1];
    const int lane = threadIdx.x;
    const uint32_t first = blockIdx.x * s.band_bytes;
    const uint32_t n = min(s.band_bytes, s.N - first);
    const uint32_t size_word = sizes[blockIdx.x], size = size_word & ~CODED_FLAG;
    const size_t dst = (size_t)offsets[blockIdx.x];
    bool overrun = false;
    if (!(size_word & CODED_FLAG)) {
        // ---- stored: blocks of at most 65535 bytes, each behind 00, its length and the length's complement
        for (uint32_t j = lane; j < size; j += WAVE) {
            const uint32_t blk = j / (STORED_MAX + 5), r = j % (STORED_MAX + 5);
            const uint32_t len = min(STORED_MAX, n - blk * STORED_MAX);
            int v;
            if (r >= 5)
                v = stream_byte(s, first + blk * STORED_MAX + (r - 5));
            else
                v = r == 0 ? 0 : (int)(((r < 3 ? len : ~len) >> (8 * ((r - 1) & 1))) & 0xFF);
            if (dst + j < capacity)
                out[dst + j] = (uint8_t)v;
            else
                overrun = true;
        }
        if (overrun)
            info[1] = 1;
        return;
    }
    const uint32_t header_bits = min(tables->header_bits, (uint32_t)MAX_HEADER_BITS);
    for (int w = lane; w < BIT_WORDS; w += WAVE)
        s_bits[w] = w < HEADER_WORDS ? tables->header[w] : 0;
    for (int w = lane; w <= END_OF_BLOCK; w += WAVE)
        s_lit[w] = tables->lit[w];
    for (int w = lane; w <= MAX_MATCH; w += WAVE)
        s_match[w] = tables->match[w];
    uint32_t bitpos = header_bits; // bits in s_bits
    uint32_t outpos = 0;           // bytes written
    int carry = 0, prev = 0;
    int cur[TRIPS], next[TRIPS];
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const uint32_t j = (uint32_t)(k * WAVE + lane);
        cur[k] = j < n ? stream_byte(s, first + j) : 0;
    }
    __syncthreads();
    for (uint32_t block = 0; block <= n; block += TRIPS * WAVE) {
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const uint32_t j = block + (uint32_t)((TRIPS + k) * WAVE + lane);
            next[k] = j < n ? stream_byte(s, first + j) : 0;
        }
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const uint32_t base = block + (uint32_t)(k * WAVE);
            if (base > n)
                break;
            const Tokens t = tokenise(cur[k], prev, base + lane, n, s.distance, lane, carry);
            prev = cur[k];
            unsigned long long bits = 0;
            int len = 0;
            if (t.match)
                put_token(bits, len, s_match[t.match]);
            if (t.pending == 2)
                put_token(bits, len, s_lit[t.older]);
            if (t.pending >= 1)
                put_token(bits, len, s_lit[t.newer]);
            if (t.own >= 0)
                put_token(bits, len, s_lit[t.own]);
            len = min(len, LANE_MAX_BITS); // (never: LANE_WORST_BITS)
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
            if (base + WAVE > n) {
                bitpos = (bitpos + 3 + 7) & ~7u;
                const uint32_t q = bitpos + 16 + 8 * (uint32_t)lane;
                if (lane < 2 && (q >> 5) < BIT_WORDS)
                    atomicOr(&s_bits[q >> 5], 0xFFu << (q & 31));
                bitpos += 32;
            }
            __syncthreads();
            // ---- the trip's whole bytes to the band's place
            const uint32_t n_bytes = bitpos >> 3;
            for (uint32_t j = lane; j < n_bytes; j += WAVE) {
                if (outpos + j < size && dst + outpos + j < capacity)
                    out[dst + outpos + j] = (uint8_t)(s_bits[j >> 2] >> (8 * (j & 3)));
                else
                    overrun = true;
            }
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
    // a band that did not come out at the size k_fz_sizes worked out has its neighbours' places wrong
    if (overrun || (lane == 0 && outpos != size))
        info[1] = 1;
}

// ---- round -------------------------------------------------------------------------------------------------------------
constexpr int ROUND_BLOCK = 256;
__device__ __forceinline__ float round_half_even(float v) { return rintf(v); }
__device__ __forceinline__ double round_half_even(double v) { return rint(v); }

template <typename T>
__global__ __launch_bounds__(ROUND_BLOCK) void k_fz_round(const T *__restrict__ in, size_t n, long long *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * ROUND_BLOCK + threadIdx.x;
    if (i >= n)
        return;
    const T r = round_half_even(in[i]); // in T
    const T edge = (T)9223372036854775808.0;
    // what does not fit, and NaN: the "integer indefinite" value the x86-64 conversion gives
    out[i] = (r >= -edge && r < edge) ? (long long)r : (long long)0x8000000000000000ull;
}

} // namespace flowzip
} // namespace tf

using namespace tf;
using namespace tf::flowzip;

struct tf_flowzip {
    uint32_t max_stream = 0, band_bytes = 0;
    int max_bands = 0;
    DevBuf consts, tables, prefix, counts, totals, band_crc, sizes, offsets, info, packed, upload;
    PinnedBuf info_host;   // page-locked unsigned long long: [0] the stream's bytes, [1] the overrun flag, [2] the CRC-32
    PinnedBuf tables_host; // page-locked Tables: the last member's tables
    size_t last_bytes = 0;                   // the stream of the last encode that ran; 0: none to copy again
};

TF_API void tf_flowzip_destroy(tf_flowzip *enc) { delete enc; }

TF_API int tf_flowzip_default_band_bytes(void)
{
    return DEFAULT_BAND_BYTES;
}

TF_API int tf_flowzip_create(tf_flowzip **out, size_t max_stream_bytes, int band_bytes)
{
    TF_REQUIRE(out, "tf_flowzip_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(max_stream_bytes >= 1 && max_stream_bytes <= ((size_t)1 << 31), "tf_flowzip_create: a stream of %zu bytes (1 to 2^31)",
               max_stream_bytes);
    TF_REQUIRE(band_bytes >= 0 && band_bytes % 64 == 0 && band_bytes <= (1 << 28),
               "tf_flowzip_create: band_bytes %d (0 = default, or a multiple of 64 up to 2^28)", band_bytes);
    // a lane's worst tokens of a trip fit its 64-bit accumulator, and 64 lanes' the LDS bit buffer behind the header
    static_assert(LANE_WORST_BITS <= LANE_MAX_BITS, "a lane's tokens outgrow its accumulator");
    static_assert(MAX_CODE_BITS + 5 + 1 + 4 < ENTRY_SHIFT, "a match outgrows its entry");
    if (MAX_HEADER_BITS + WAVE * LANE_WORST_BITS + 3 + 7 + 32 > 32 * (BIT_WORDS - 3))
        return set_error(TF_ERR_STATE, "tf_flowzip_create: a trip's tokens would not fit the bit buffer");
    TF_TRY(ensure_init());
    auto enc = make_handle<tf_flowzip>();
    TF_REQUIRE(enc, "tf_flowzip_create: out of memory");
    enc->max_stream = (uint32_t)max_stream_bytes;
    enc->band_bytes = band_bytes ? (uint32_t)band_bytes : (uint32_t)DEFAULT_BAND_BYTES;
    enc->max_bands = (int)((max_stream_bytes + enc->band_bytes - 1) / enc->band_bytes);
    const size_t n = (size_t)enc->max_bands;
    Crc32Consts consts;
    make_crc32_consts(consts);
    TF_TRY(enc->consts.alloc(sizeof(Crc32Consts)));
    TF_TRY(enc->tables.alloc(sizeof(Tables)));
    TF_TRY(enc->prefix.alloc(MAX_PREFIX_BYTES));
    TF_TRY(enc->counts.alloc(n * N_SYMBOLS * sizeof(uint32_t)));
    TF_TRY(enc->totals.alloc(N_SYMBOLS * sizeof(uint32_t)));
    TF_TRY(enc->band_crc.alloc(n * sizeof(uint32_t)));
    TF_TRY(enc->sizes.alloc(n * sizeof(uint32_t)));
    TF_TRY(enc->offsets.alloc(n * sizeof(unsigned long long)));
    TF_TRY(enc->info.alloc(4 * sizeof(unsigned long long)));
    TF_TRY(enc->packed.alloc((size_t)stream_bound(max_stream_bytes, enc->band_bytes))); // the bound: every band stored
    TF_TRY(enc->info_host.alloc(4 * sizeof(unsigned long long)));
    TF_TRY(enc->tables_host.alloc(sizeof(Tables)));
    TF_HIP(hipMemcpyAsync(enc->consts.p, &consts, sizeof(Crc32Consts), hipMemcpyHostToDevice, stream()));
    TF_HIP(hipStreamSynchronize(stream())); // `consts` is on this stack
    *out = enc.release();
    return TF_OK;
}

TF_API int tf_flowzip_band_bytes(tf_flowzip *enc)
{
    return enc ? (int)enc->band_bytes : 0;
}

// the stream to the caller, if it fits; *n_bytes either way
static int copy_out(tf_flowzip *enc, const char *who, uint8_t *out, size_t capacity, size_t *n_bytes)
{
    *n_bytes = enc->last_bytes;
    TF_REQUIRE(*n_bytes <= capacity, "%s: the stream has %zu bytes, the buffer %zu", who, *n_bytes, capacity);
    TF_HIP(hipMemcpyAsync(out, enc->packed.p, enc->last_bytes, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

TF_API int tf_flowzip_encode_dev(tf_flowzip *enc, const uint8_t *prefix_host, size_t prefix_len, const void *data_dev, size_t data_bytes,
                                 int distance, uint8_t *out, size_t capacity, size_t *n_bytes, uint32_t *crc32)
{
    TF_REQUIRE(enc && n_bytes && crc32 && (out || capacity == 0) && (prefix_host || prefix_len == 0) && (data_dev || data_bytes == 0),
               "tf_flowzip_encode_dev: null pointer");
    *n_bytes = 0, *crc32 = 0;
    TF_REQUIRE(prefix_len % 64 == 0 && prefix_len <= MAX_PREFIX_BYTES,
               "tf_flowzip_encode_dev: a prefix of %zu bytes (a multiple of 64, at most %d)", prefix_len, MAX_PREFIX_BYTES);
    TF_REQUIRE(distance >= 1 && distance <= MAX_DISTANCE, "tf_flowzip_encode_dev: distance %d (1 to %d)", distance, MAX_DISTANCE);
    TF_REQUIRE(data_bytes <= enc->max_stream && prefix_len + data_bytes >= 1 && prefix_len + data_bytes <= enc->max_stream,
               "tf_flowzip_encode_dev: a stream of %zu bytes, the handle is for 1 to %u", prefix_len + data_bytes, enc->max_stream);
    enc->last_bytes = 0;
    Stream s;
    s.prefix = enc->prefix.as<uint8_t>(), s.data = (const uint8_t *)data_dev, s.prefix_len = (uint32_t)prefix_len;
    s.N = (uint32_t)(prefix_len + data_bytes), s.band_bytes = enc->band_bytes, s.distance = distance;
    const int n_bands = (int)(((size_t)s.N + s.band_bytes - 1) / s.band_bytes); // (at most max_bands)
    if (prefix_len)
        TF_HIP(hipMemcpyAsync(enc->prefix.p, prefix_host, prefix_len, hipMemcpyHostToDevice, stream()));
    TF_HIP(hipMemsetAsync(enc->info.p, 0, enc->info.bytes, stream()));
    TF_HIP(hipMemsetAsync(enc->totals.p, 0, enc->totals.bytes, stream()));
    TF_TRY(launch("fz_count", k_fz_count, dim3(n_bands), dim3(WAVE), 0, s, enc->consts.as<Crc32Consts>(), enc->counts.as<uint32_t>(),
                  enc->totals.as<uint32_t>(), enc->band_crc.as<uint32_t>()));
    TF_TRY(launch("fz_table", k_fz_table, dim3(1), dim3(TABLE_BLOCK), 0, enc->totals.as<uint32_t>(), distance, enc->tables.as<Tables>()));
    TF_TRY(launch("fz_sizes", k_fz_sizes, dim3(cdiv(n_bands, SIZES_BLOCK / WAVE)), dim3(SIZES_BLOCK), 0, enc->counts.as<uint32_t>(),
                  enc->tables.as<Tables>(), s.N, s.band_bytes, n_bands, enc->sizes.as<uint32_t>()));
    TF_TRY(launch("fz_scan", k_fz_scan, dim3(1), dim3(SCAN_BLOCK), 0, enc->sizes.as<uint32_t>(), enc->offsets.as<unsigned long long>(),
                  n_bands, enc->band_crc.as<uint32_t>(), enc->consts.as<Crc32Consts>(), s.N, s.band_bytes, enc->packed.as<uint8_t>(),
                  enc->packed.bytes, enc->info.as<unsigned long long>()));
    TF_TRY(launch("fz_emit", k_fz_emit, dim3(n_bands), dim3(WAVE), 0, s, enc->tables.as<Tables>(), enc->sizes.as<uint32_t>(),
                  enc->offsets.as<unsigned long long>(), enc->packed.as<uint8_t>(), enc->packed.bytes,
                  enc->info.as<unsigned long long>()));
    TF_HIP(hipMemcpyAsync(enc->info_host.p, enc->info.p, enc->info.bytes, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipMemcpyAsync(enc->tables_host.p, enc->tables.p, sizeof(Tables), hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    const unsigned long long *info = enc->info_host.as<unsigned long long>();
    if (info[1] || info[0] > enc->packed.bytes)
        return set_error(TF_ERR_STATE, "tf_flowzip_encode_dev: the stream outgrew its buffer of %zu bytes", enc->packed.bytes);
    enc->last_bytes = (size_t)info[0];
    *crc32 = (uint32_t)info[2];
    return copy_out(enc, "tf_flowzip_encode_dev", out, capacity, n_bytes);
}

TF_API int tf_flowzip_encode(tf_flowzip *enc, const uint8_t *prefix_host, size_t prefix_len, const void *data_host, size_t data_bytes,
                             int distance, uint8_t *out, size_t capacity, size_t *n_bytes, uint32_t *crc32)
{
    TF_REQUIRE(enc && n_bytes && crc32 && (data_host || data_bytes == 0), "tf_flowzip_encode: null pointer");
    *n_bytes = 0, *crc32 = 0;
    TF_REQUIRE(data_bytes <= enc->max_stream, "tf_flowzip_encode: %zu bytes of data, the handle is for streams of %u", data_bytes,
               enc->max_stream);
    if (!enc->upload.p)
        TF_TRY(enc->upload.alloc(enc->max_stream)); // once, for the longest stream: nothing below grows it
    if (data_bytes)
        TF_TRY(enc->upload.upload(data_host, data_bytes));
    return tf_flowzip_encode_dev(enc, prefix_host, prefix_len, enc->upload.p, data_bytes, distance, out, capacity, n_bytes, crc32);
}

TF_API int tf_flowzip_copy_last(tf_flowzip *enc, uint8_t *out, size_t capacity, size_t *n_bytes)
{
    TF_REQUIRE(enc && n_bytes && (out || capacity == 0), "tf_flowzip_copy_last: null pointer");
    *n_bytes = 0;
    if (!enc->last_bytes)
        return set_error(TF_ERR_STATE, "tf_flowzip_copy_last: nothing has been encoded");
    return copy_out(enc, "tf_flowzip_copy_last", out, capacity, n_bytes);
}

TF_API int tf_flowzip_last_lengths(tf_flowzip *enc, uint8_t *out)
{
    TF_REQUIRE(enc && out, "tf_flowzip_last_lengths: null pointer");
    if (!enc->last_bytes)
        return set_error(TF_ERR_STATE, "tf_flowzip_last_lengths: nothing has been encoded");
    memcpy(out, enc->tables_host.as<Tables>()->lengths, N_SYMBOLS);
    return TF_OK;
}

TF_API int tf_flowzip_last_band_sizes(tf_flowzip *enc, uint32_t *out, size_t capacity, size_t *n_bands)
{
    TF_REQUIRE(enc && n_bands && (out || capacity == 0), "tf_flowzip_last_band_sizes: null pointer");
    *n_bands = 0;
    if (!enc->last_bytes)
        return set_error(TF_ERR_STATE, "tf_flowzip_last_band_sizes: nothing has been encoded");
    // the handle keeps no band count: the bands are those whose sizes sum to the stream without its final block (a band
    // has at least six bytes, so the sum reaches that value once)
    // (a block of the handle's size words at a time, so that nothing here allocates)
    constexpr size_t CHUNK = 1024;
    uint32_t words[CHUNK];
    const size_t max_bands = (size_t)enc->max_bands;
    size_t n = 0, sum = 0;
    for (size_t base = 0; base < max_bands && sum + 5 < enc->last_bytes; base += CHUNK) {
        const size_t count = max_bands - base < CHUNK ? max_bands - base : CHUNK;
        TF_HIP(hipMemcpyAsync(words, enc->sizes.as<uint32_t>() + base, count * sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
        TF_HIP(hipStreamSynchronize(stream()));
        for (size_t k = 0; k < count && sum + 5 < enc->last_bytes; k++, n++) {
            const uint32_t size = words[k] & ~CODED_FLAG;
            sum += size;
            if (n < capacity)
                out[n] = size;
        }
    }
    if (sum + 5 != enc->last_bytes)
        return set_error(TF_ERR_STATE, "tf_flowzip_last_band_sizes: the bands' sizes do not sum to the stream's");
    *n_bands = n;
    TF_REQUIRE(n <= capacity, "tf_flowzip_last_band_sizes: %zu bands, room for %zu", n, capacity);
    return TF_OK;
}

TF_API int tf_flow_round_i64_dev(const void *flow_dev, size_t n_values, int wide, void *out_dev)
{
    TF_REQUIRE((flow_dev && out_dev) || n_values == 0, "tf_flow_round_i64_dev: null pointer");
    TF_REQUIRE(n_values <= ((size_t)1 << 32), "tf_flow_round_i64_dev: %zu values (at most 2^32)", n_values);
    TF_TRY(ensure_init());
    const dim3 grid(cdiv(n_values, ROUND_BLOCK)), block(ROUND_BLOCK);
    if (wide)
        return launch("fz_round", k_fz_round<double>, grid, block, 0, (const double *)flow_dev, n_values, (long long *)out_dev);
    return launch("fz_round", k_fz_round<float>, grid, block, 0, (const float *)flow_dev, n_values, (long long *)out_dev);
}
