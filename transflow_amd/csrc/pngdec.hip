// Banded PNG frames decoded where the frame is wanted (tests/pngdec_ref.py is the Python
// statement of the same rules).  The file is PngEncoder(index=True)'s kind (pngdec_common.h): the host walks its chunks,
// the compressed file goes up as it is, and everything else runs on the library stream.
//
//   k_pd_crc       one wave per band: the CRC-32 of the chunk's type and compressed bytes by slices (crc32_common.h),
//                  compared with the four bytes behind them; the lowest chunk that differs goes to the status words.
//   k_pd_inflate   one wave per band over the machine of flowunzip_common.h, with k_fu_inflate's contract and loop: lane
//                  0 runs the machine over a window of the band's bytes and a ring of its last 32768 bytes, both in LDS,
//                  and the wave refills, copies and flushes.  A match reads the ring, never the destination.  Band b
//                  inflates into slot b of the filtered-rows buffer; a band is rows * (1 + 3 W) bytes, no multiple of
//                  64, so the slots' stride is that rounded up to 16 and the last flush ends in single bytes.  Every
//                  load is checked against the band's compressed range, every store against its slot, every ring index
//                  is masked.  A rejected band leaves (band << 8 | reason) in the status words, the lowest band wins.
//   k_pd_rows      one work-group per row: the filter type must be 0 - 4 (the lowest bad row goes to the status words),
//                  and the row's two Adler sums as k_png_filter makes them (64-bit, reduced once) for the host to combine.
//   k_pd_unfilter  one wave per segment.  A segment begins at row 0 and at every None or Sub row -- rows that do not read
//                  the row above -- and runs to the row before the next such row.  Wave y looks at row y's type and
//                  leaves unless the row begins a segment; no wave waits for another, and segments touch disjoint rows.
//                  The wave marches MARCH_ROWS = 64 rows together, lane l on row base + l, each lane one chunk of four
//                  pixels behind the lane above: at step t lane l undoes chunk t - l.  b (above) comes from the lane
//                  above by a cross-lane move of the three dwords it made one step earlier, c (above-left) and a (left)
//                  stay in registers from the chunk before.  A lane loads its filtered bytes as aligned dwords one step
//                  ahead of their use and stores its pixels as three dwords where the row's place allows.
//                  A segment longer than 64 rows is walked in blocks.  Lane 0 of a later block needs the pixels lane 63
//                  of the block before stored -- the hazard: a load of global memory that another lane of the same wave
//                  has stored.  It is closed by the barrier at the end of every block: __syncthreads() waits for the
//                  wave's stores and orders them, at work-group scope, before the loads that follow, and the work-group
//                  is this one wave.  This relies on the default CU mode the library is built for: a work-group lives on
//                  one compute unit, so its stores and later loads meet in that unit's vector L1 and work-group scope
//                  is enough.  In threadgroup-split mode (-mtgsplit, which no unit here uses) a work-group's scope spans
//                  compute units and the code would have to be compiled for that mode to stay ordered.  The row is then read 64 chunks at a time by all lanes and handed to lane 0 by a
//                  cross-lane move.  No loop's trip count depends on the file: they are bounded by H and W, which the
//                  host checked, and the types are read from the slots, which are the handle's.
#include "pngdec_common.h"

#include "common.h"

#include <cstring>
#include <new>

namespace tf {
namespace pngdec {

using flowunzip::Action;
using flowunzip::Code;
using flowunzip::State;

constexpr int WAVE = 64;
constexpr uint32_t ST_NONE = 0xFFFFFFFFu;
enum StatusWord { ST_CRC = 0, ST_BAND = 1, ST_FILTER = 2, ST_WORDS = 4 };
constexpr uint32_t SLOT_ALIGN = 16;
constexpr uint32_t FILT_PAD = 16;  // behind the last slot: the unfilter kernel's dword loads may reach past a row's end
constexpr uint32_t ADLER_BASE = 65521;

struct Frame {
    const uint8_t *file; // the whole file in device memory
    uint32_t file_bytes;
    const uint32_t *band_off, *band_size; // n_bands each: a band's compressed bytes in the file
    uint32_t n_bands, band_rows, W, H, row_len, first_band_chunk;
    uint8_t *filt; // n_bands slots slot_stride bytes apart (the last as long as its rows), and FILT_PAD
    uint32_t slot_stride;
    size_t filt_bytes;
};

__device__ __forceinline__ uint32_t rows_of_band(const Frame &f, uint32_t band)
{
    const uint32_t first = band * f.band_rows; // (band < n_bands: below H)
    return min(f.band_rows, f.H - first);
}

// ---- chunk CRCs ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_pd_crc(const Frame f, const Crc32Consts *__restrict__ consts, uint32_t *__restrict__ status)
{
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_x2n[32];
    const int lane = threadIdx.x;
    crc32_stage_table(s_crc, consts, lane, WAVE);
    crc32_stage_x2n(s_x2n, consts, lane);
    __syncthreads();
    const uint32_t band = blockIdx.x;
    const uint32_t off = f.band_off[band], size = f.band_size[band];
    if (off < 4 || off > f.file_bytes || size > f.file_bytes - off || f.file_bytes - off - size < 4) { // (never: the host's walk)
        if (lane == 0)
            atomicMin(&status[ST_CRC], f.first_band_chunk + band);
        return;
    }
    const uint8_t *p = f.file + (off - 4); // the type, then the data
    const uint32_t n = size + 4;           // (size <= 2^32 - 13)
    const uint32_t slice = (n + WAVE - 1) / WAVE;
    const uint32_t begin = min((uint32_t)lane * slice, n), end = min(begin + slice, n);
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t j = begin; j < end; j++)
        c = crc32_update(c, p[j], s_crc);
    c = crc32_wave_xor(crc32_shift(~c, n - end, s_x2n)); // ~c: the slice's own CRC-32 (of no bytes: 0)
    const uint32_t stored = be32(p + n);
    if (lane == 0 && c != stored)
        atomicMin(&status[ST_CRC], f.first_band_chunk + band);
}

// ---- inflate ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void reject_band(uint32_t *status, uint32_t band, uint32_t why)
{
    atomicMin(&status[ST_BAND], (band << 8) | why);
}

__global__ __launch_bounds__(WAVE) void k_pd_inflate(const Frame f, uint32_t *__restrict__ status)
{
    using namespace flowunzip;
    __shared__ uint32_t s_ring[RING_BYTES / 4];
    __shared__ uint32_t s_win[WINDOW_BYTES / 4];
    __shared__ Code s_lit, s_dist;
    __shared__ uint32_t s_lengths[MAX_LENGTHS / 4];
    uint8_t *ring = reinterpret_cast<uint8_t *>(s_ring);
    uint8_t *win = reinterpret_cast<uint8_t *>(s_win);
    const int lane = threadIdx.x;
    const uint32_t band = blockIdx.x;
    const uint32_t out_bytes = rows_of_band(f, band) * f.row_len; // (at most 2^28: tf_pngdec_decode_dev)
    const uint32_t off = f.band_off[band], size = f.band_size[band];
    uint8_t *slot = f.filt + (size_t)band * f.slot_stride; // 16-byte aligned
    if (off > f.file_bytes || size > f.file_bytes - off || out_bytes > f.slot_stride) { // (never: the host makes them)
        if (lane == 0)
            reject_band(status, band, R_EXHAUSTED);
        return;
    }
    const uint8_t *src = f.file + off;
    State s;
    start(s, win, size, out_bytes);
    for (;;) {
        Action x = make_action(A_DONE, flowunzip::R_OK, 0, 0);
        if (lane == 0)
            x = advance(s, s_lit, s_dist, reinterpret_cast<uint8_t *>(s_lengths), ring);
        x.kind = __shfl(x.kind, 0, WAVE), x.a = __shfl(x.a, 0, WAVE), x.b = __shfl(x.b, 0, WAVE), x.c = __shfl(x.c, 0, WAVE);
        const uint32_t produced = __shfl(s.produced, 0, WAVE), flushed = __shfl(s.flushed, 0, WAVE);
        __syncthreads(); // lane 0's literals are in the ring
        if (x.kind == A_REFILL) {
#pragma unroll
            for (uint32_t k = 0; k < WINDOW_BYTES / WAVE; k++) { // a fixed count: the loads go out together
                const uint32_t i = k * WAVE + lane;
                uint8_t v = 0;
                if (i < x.b && x.a <= size && i < size - x.a)
                    v = src[x.a + i];
                if (i < x.b && i < WINDOW_BYTES)
                    win[i] = v;
            }
        } else if (x.kind == A_MATCH) {
            const uint32_t at = x.a, len = x.b, d = x.c;
            if (d == 0 || d > at || d > RING_BYTES || len > 258 || len > out_bytes - min(at, out_bytes)) { // (never: step checked)
                if (lane == 0)
                    reject_band(status, band, R_DISTANCE);
                return;
            }
            // byte j of the match is byte j mod d of the d bytes in front of it: every source is older than the match
            for (uint32_t base = 0; base < len; base += WAVE) {
                const uint32_t j = base + lane;
                uint8_t v = 0;
                if (j < len)
                    v = ring[(at - d + (j < d ? j : j % d)) & RING_MASK];
                __syncthreads(); // a byte's slot is also that of the byte 32768 before it: read before any lane writes
                if (j < len)
                    ring[(at + j) & RING_MASK] = v;
            }
        } else if (x.kind == A_STORED) {
#pragma unroll
            for (uint32_t k = 0; k < STORED_CHUNK / WAVE; k++) {
                const uint32_t i = k * WAVE + lane;
                const bool mine = i < x.b && x.c <= size && i < size - x.c && x.a <= out_bytes && i < out_bytes - x.a;
                uint8_t v = 0;
                if (mine)
                    v = src[x.c + i];
                if (mine)
                    ring[(x.a + i) & RING_MASK] = v;
            }
        } else if (x.kind == A_FLUSH || (x.kind == A_DONE && x.a == flowunzip::R_OK)) {
            const uint32_t upto = x.kind == A_DONE ? produced : produced & ~63u; // flushed is a multiple of 64
            if (upto > out_bytes || flushed > upto || upto - flushed > RING_BYTES) { // (never)
                if (lane == 0)
                    reject_band(status, band, R_OVERRUN);
                return;
            }
            // whole words while they last (the slot and `flushed` are word-aligned), the band's unaligned end byte by byte
            const uint32_t words_end = flushed + ((upto - flushed) & ~3u);
            for (uint32_t w = flushed + 4 * (uint32_t)lane; w < words_end; w += 4 * WAVE)
                if (w + 4 <= out_bytes)
                    *reinterpret_cast<uint32_t *>(slot + w) = s_ring[(w & RING_MASK) >> 2];
            for (uint32_t i = words_end + lane; i < upto; i += WAVE)
                if (i < out_bytes)
                    slot[i] = ring[i & RING_MASK];
            if (lane == 0)
                s.flushed = upto;
        }
        if (x.kind == A_DONE) {
            if (lane == 0 && x.a != flowunzip::R_OK)
                reject_band(status, band, x.a);
            return;
        }
        __syncthreads(); // the wave's bytes are in LDS before lane 0 goes on
    }
}

// ---- rows: the filter types, the Adler sums ----------------------------------------------------------------------------
__device__ __forceinline__ const uint8_t *row_of(const Frame &f, uint32_t y) // y < H
{
    const uint32_t band = y / f.band_rows;
    return f.filt + (size_t)band * f.slot_stride + (size_t)(y - band * f.band_rows) * f.row_len;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int d = WAVE / 2; d; d >>= 1)
        v += __shfl_xor(v, d, WAVE);
    return v;
}

constexpr int ROWS_BLOCK = 256;
// rowsums[2 r], [2 r + 1]: the sum of the filtered row's L bytes and the sum of (L - j) byte[j], both mod 65521
// (255 L (L + 1) / 2 < 2^56 for L <= 3 * 2^24 + 1: nothing is reduced before the end)
__global__ __launch_bounds__(ROWS_BLOCK) void k_pd_rows(const Frame f, uint32_t *__restrict__ rowsums, uint32_t *__restrict__ status)
{
    __shared__ unsigned long long s_adler[ROWS_BLOCK / WAVE][2];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const uint32_t y = blockIdx.x;
    const uint8_t *row = row_of(f, y);
    const uint32_t L = f.row_len;
    if (tid == 0 && row[0] > 4)
        atomicMin(&status[ST_FILTER], y);
    unsigned long long s1 = 0, s2 = 0;
    for (uint32_t j = tid; j < L; j += ROWS_BLOCK) {
        const unsigned long long v = row[j];
        s1 += v;
        s2 += v * (L - j);
    }
    s1 = wave_sum64(s1), s2 = wave_sum64(s2);
    if (lane == 0)
        s_adler[wave][0] = s1, s_adler[wave][1] = s2;
    __syncthreads();
    if (tid == 0) {
        s1 = s2 = 0;
        for (int w = 0; w < ROWS_BLOCK / WAVE; w++)
            s1 += s_adler[w][0], s2 += s_adler[w][1];
        rowsums[2 * (size_t)y] = (uint32_t)(s1 % ADLER_BASE);
        rowsums[2 * (size_t)y + 1] = (uint32_t)(s2 % ADLER_BASE);
    }
}

// ---- unfilter --------------------------------------------------------------------------------------------------------
constexpr uint32_t CHUNK_PX = 4, CHUNK_BYTES = 3 * CHUNK_PX;
static_assert(MARCH_ROWS == WAVE, "a lane a row");

// the four aligned dwords that hold the twelve bytes from p on; nothing outside [lo, hi) is read
__device__ __forceinline__ void load_raw(const uint8_t *p, const uint8_t *lo, const uint8_t *hi, uint32_t w[4])
{
    const uint8_t *q = p - ((uintptr_t)p & 3);
#pragma unroll
    for (int i = 0; i < 4; i++)
        w[i] = (q + 4 * i >= lo && q + 4 * i + 4 <= hi) ? *reinterpret_cast<const uint32_t *>(q + 4 * i) : 0;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t d[3], int j) { return (d[j >> 2] >> (8 * (j & 3))) & 0xFFu; }

// RGB <-> BGR of four packed pixels: bytes 0 and 2 of every three change places
__device__ __forceinline__ void swap_rb(const uint32_t in[3], uint32_t out[3])
{
    out[0] = out[1] = out[2] = 0;
#pragma unroll
    for (int j = 0; j < 12; j++) {
        const int from = j - j % 3 + (2 - j % 3);
        out[j >> 2] |= byte_of(in, from) << (8 * (j & 3));
    }
}

__global__ __launch_bounds__(WAVE) void k_pd_unfilter(const Frame f, uint8_t *__restrict__ pix, int bgr, const uint32_t *__restrict__ status)
{
    const int lane = threadIdx.x;
    if (status[ST_BAND] != ST_NONE || status[ST_FILTER] != ST_NONE) // written by kernels that have ended
        return;
    const uint32_t y0 = blockIdx.x; // (below H: the grid)
    const uint32_t t0 = row_of(f, y0)[0];
    if (y0 != 0 && t0 >= 2) // a row inside a segment (t0 <= 4: k_pd_rows found no other)
        return;
    const uint32_t W = f.W, H = f.H;
    const size_t pix_row = 3 * (size_t)W;
    const uint32_t n_chunks = (W + CHUNK_PX - 1) / CHUNK_PX;
    const uint8_t *lo = f.filt, *hi = f.filt + f.filt_bytes;
    for (uint32_t base = y0; base < H; base += WAVE) { // at most ceil(H / 64) trips
        const uint32_t y = base + (uint32_t)lane;
        const bool in_image = y < H; // (base + 63 < 2^25)
        const uint8_t *row = in_image ? row_of(f, y) : f.filt;
        const uint32_t type = in_image ? row[0] : 0;
        // the block's rows: up to the first row that begins another segment, or the image's end
        const unsigned long long stop = __ballot(!in_image || (y != y0 && type < 2));
        const uint32_t n_rows = stop ? (uint32_t)__ffsll((long long)stop) - 1 : (uint32_t)WAVE;
        if (n_rows == 0)
            break;
        const bool active = (uint32_t)lane < n_rows;
        const bool has_above = base > y0; // the block before stored that row; a segment's first row reads none
        const uint8_t *above = has_above ? pix + (size_t)(base - 1) * pix_row : pix;
        uint8_t *dst = pix + (size_t)(active ? y : base) * pix_row;
        const uint8_t *src = row + 1;
        const uint32_t sh = 8 * (uint32_t)((uintptr_t)src & 3); // (CHUNK_BYTES is a multiple of 4: the same for every chunk)
        uint32_t nx[4] = {0, 0, 0, 0};
        if (active)
            load_raw(src, lo, hi, nx);
        uint32_t out[3] = {0, 0, 0};   // the chunk this lane made one step ago, RGB
        uint32_t batch[3] = {0, 0, 0}; // lane j: chunk (t & ~63) + j of the row above the block, RGB
        uint32_t a_prev = 0, c_prev = 0; // the pixel left of the chunk, in this row and in the row above (bytes 0 - 2)
        const uint32_t steps = n_chunks + n_rows - 1;
        for (uint32_t t = 0; t < steps; t++) {
            if ((t & 63u) == 0) {
                batch[0] = batch[1] = batch[2] = 0;
                const uint32_t k = t + (uint32_t)lane;
                if (has_above && k < n_chunks) {
                    uint32_t raw[3] = {0, 0, 0};
#pragma unroll
                    for (int j = 0; j < (int)CHUNK_BYTES; j++)
                        if (CHUNK_PX * k + j / 3 < W)
                            raw[j >> 2] |= (uint32_t)above[(size_t)CHUNK_BYTES * k + j] << (8 * (j & 3));
                    if (bgr)
                        swap_rb(raw, batch);
                    else
                        batch[0] = raw[0], batch[1] = raw[1], batch[2] = raw[2];
                }
            }
            uint32_t b[3];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const uint32_t up = __shfl_up(out[i], 1, WAVE);
                const uint32_t first = __shfl(batch[i], (int)(t & 63u), WAVE);
                b[i] = lane == 0 ? first : up;
            }
            const uint32_t k = t - (uint32_t)lane;
            if (active && t >= (uint32_t)lane && k < n_chunks) {
                uint32_t x[3];
#pragma unroll
                for (int i = 0; i < 3; i++)
                    x[i] = __funnelshift_r(nx[i], nx[i + 1], sh);
                if (k + 1 < n_chunks)
                    load_raw(src + (size_t)CHUNK_BYTES * (k + 1), lo, hi, nx);
                uint32_t o[3] = {0, 0, 0};
                uint32_t a[3] = {a_prev & 0xFFu, (a_prev >> 8) & 0xFFu, (a_prev >> 16) & 0xFFu};
                uint32_t c[3] = {c_prev & 0xFFu, (c_prev >> 8) & 0xFFu, (c_prev >> 16) & 0xFFu};
#pragma unroll
                for (int j = 0; j < (int)CHUNK_BYTES; j++) {
                    const uint32_t bj = byte_of(b, j);
                    const uint32_t v = unfilter_byte(type, byte_of(x, j), a[j % 3], bj, c[j % 3]);
                    a[j % 3] = v, c[j % 3] = bj;
                    o[j >> 2] |= v << (8 * (j & 3));
                }
                a_prev = a[0] | (a[1] << 8) | (a[2] << 16);
                c_prev = c[0] | (c[1] << 8) | (c[2] << 16);
                out[0] = o[0], out[1] = o[1], out[2] = o[2];
                uint32_t q[3];
                if (bgr)
                    swap_rb(o, q);
                else
                    q[0] = o[0], q[1] = o[1], q[2] = o[2];
                uint8_t *d = dst + (size_t)CHUNK_BYTES * k;
                if (CHUNK_PX * k + CHUNK_PX <= W && ((uintptr_t)d & 3) == 0) {
                    uint32_t *d4 = reinterpret_cast<uint32_t *>(d);
                    d4[0] = q[0], d4[1] = q[1], d4[2] = q[2];
                } else {
#pragma unroll
                    for (int j = 0; j < (int)CHUNK_BYTES; j++)
                        if (CHUNK_PX * k + j / 3 < W) // nothing beyond the row's W pixels
                            d[j] = (uint8_t)byte_of(q, j);
                }
            }
        }
        if (n_rows < (uint32_t)WAVE)
            break;
        __syncthreads(); // the block's stores are done and ordered before the next block's loads of its last row
    }
}

} // namespace pngdec
} // namespace tf

using namespace tf;
using namespace tf::pngdec;

struct tf_pngdec {
    int max_w = 0, max_h = 0;
    size_t max_file = 0, filt_bytes = 0;
    Crc32Consts consts;
    DevBuf dev_consts, file, bands, filt, rowsums, status, out;
    PinnedBuf stage;        // page-locked uint8_t: the file on its way up
    PinnedBuf bands_host;   // page-locked uint32_t: max_h offsets, then max_h sizes
    PinnedBuf rowsums_host; // page-locked uint32_t
    PinnedBuf status_host;  // page-locked uint32_t
    Layout layout;
    flowunzip::Code lit, dist; // the walk's working space (the tail's block)
    uint8_t lengths[flowunzip::MAX_LENGTHS];
};

TF_API const char *tf_pngdec_reject_name(uint32_t reject) { return reject_name(reject); }

static void fill_info(tf_pngdec_info *info, const Layout &l, uint32_t reject)
{
    info->width = (int)l.width, info->height = (int)l.height, info->band_rows = (int)l.band_rows, info->n_bands = (int)l.n_bands;
    info->indexed = (int)l.indexed, info->why_not = (int)l.why_not;
    info->reject = reject, info->max_band_bytes = l.max_band_bytes;
}

TF_API int tf_pngdec_probe(const uint8_t *file, size_t n, tf_pngdec_info *info)
{
    TF_REQUIRE((file || n == 0) && info, "tf_pngdec_probe: null pointer");
    TF_REQUIRE((info->band_offsets && info->band_sizes) || info->band_capacity == 0, "tf_pngdec_probe: band_capacity %zu without arrays",
               info->band_capacity);
    static thread_local flowunzip::Code lit, dist; // the walker's working space, one per calling thread
    static thread_local uint8_t lengths[flowunzip::MAX_LENGTHS];
    Layout l;
    const uint32_t r = walk(file, n, MAX_DIM, MAX_DIM, l, info->band_offsets, info->band_sizes, info->band_capacity, lit, dist, lengths);
    fill_info(info, l, r);
    return TF_OK;
}

TF_API void tf_pngdec_destroy(tf_pngdec *dec) { delete dec; }

TF_API int tf_pngdec_create(tf_pngdec **out, int max_width, int max_height, size_t max_file_bytes)
{
    TF_REQUIRE(out, "tf_pngdec_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(max_width >= 1 && max_height >= 1 && (uint32_t)max_width <= MAX_DIM && (uint32_t)max_height <= MAX_DIM,
               "tf_pngdec_create: bad size %dx%d (1 to %u)", max_width, max_height, MAX_DIM);
    TF_REQUIRE(row_bytes((uint32_t)max_width) * (uint64_t)max_height <= MAX_STREAM, "tf_pngdec_create: %dx%d is more than 2^31 filtered bytes",
               max_width, max_height);
    TF_REQUIRE(max_file_bytes >= 1 && max_file_bytes <= ((size_t)1 << 31), "tf_pngdec_create: a file of %zu bytes (1 to 2^31)", max_file_bytes);
    TF_TRY(ensure_init());
    auto dec = make_handle<tf_pngdec>();
    TF_REQUIRE(dec, "tf_pngdec_create: out of memory");
    dec->max_w = max_width, dec->max_h = max_height, dec->max_file = max_file_bytes;
    // the bands' bytes, each but the last rounded up to SLOT_ALIGN: at most H rows' bytes and SLOT_ALIGN a band
    dec->filt_bytes = (size_t)max_height * ((size_t)row_bytes((uint32_t)max_width) + SLOT_ALIGN) + FILT_PAD;
    make_crc32_consts(dec->consts);
    const size_t h = (size_t)max_height;
    TF_TRY(dec->dev_consts.alloc(sizeof(Crc32Consts)));
    TF_TRY(dec->file.alloc(max_file_bytes + 4));
    TF_TRY(dec->bands.alloc(2 * h * sizeof(uint32_t)));
    TF_TRY(dec->filt.alloc(dec->filt_bytes));
    TF_TRY(dec->rowsums.alloc(2 * h * sizeof(uint32_t)));
    TF_TRY(dec->status.alloc(ST_WORDS * sizeof(uint32_t)));
    TF_TRY(dec->stage.alloc(max_file_bytes));
    TF_TRY(dec->bands_host.alloc(2 * h * sizeof(uint32_t)));
    TF_TRY(dec->rowsums_host.alloc(2 * h * sizeof(uint32_t)));
    TF_TRY(dec->status_host.alloc(ST_WORDS * sizeof(uint32_t)));
    TF_HIP(hipMemcpyAsync(dec->dev_consts.p, &dec->consts, sizeof(Crc32Consts), hipMemcpyHostToDevice, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    *out = dec.release();
    return TF_OK;
}

static int rejected(uint32_t *reject, uint32_t word)
{
    *reject = word;
    return set_error(TF_ERR_STATE, "tf_pngdec_decode_dev: the file is rejected: %s (at %u)", reject_name(word), word >> 8);
}

TF_API int tf_pngdec_decode_dev(tf_pngdec *dec, const uint8_t *file, size_t n, void *pix_dev, int bgr, uint32_t *reject)
{
    TF_REQUIRE(dec && (file || n == 0) && pix_dev && reject, "tf_pngdec_decode_dev: null pointer");
    TF_REQUIRE(bgr == 0 || bgr == 1, "tf_pngdec_decode_dev: bgr %d (0 RGB, 1 BGR)", bgr);
    *reject = R_OK;
    TF_REQUIRE(n <= dec->max_file, "tf_pngdec_decode_dev: a file of %zu bytes, the handle is for %zu", n, dec->max_file);
    Layout &l = dec->layout;
    uint32_t *band_off = dec->bands_host.as<uint32_t>(), *band_size = band_off + dec->max_h;
    uint32_t r = walk(file, n, (uint32_t)dec->max_w, (uint32_t)dec->max_h, l, band_off, band_size, (size_t)dec->max_h, dec->lit, dec->dist,
                      dec->lengths);
    if (r != R_OK)
        return rejected(reject, r);
    TF_REQUIRE(l.indexed, "tf_pngdec_decode_dev: a PNG without a band index, or not 8-bit RGB, or interlaced, is not for the device (%u)",
               l.why_not);
    const uint64_t L = row_bytes(l.width);
    TF_REQUIRE((uint64_t)l.band_rows * L <= (1u << 28), "tf_pngdec_decode_dev: a band of %u rows has %llu bytes (at most 2^28)", l.band_rows,
               (unsigned long long)((uint64_t)l.band_rows * L));
    r = check_small_crcs(file, n, l, dec->consts);
    if (r != R_OK)
        return rejected(reject, r);
    Frame f;
    f.file = dec->file.as<uint8_t>(), f.file_bytes = (uint32_t)n;
    f.band_off = dec->bands.as<uint32_t>(), f.band_size = dec->bands.as<uint32_t>() + dec->max_h;
    f.n_bands = l.n_bands, f.band_rows = l.band_rows, f.W = l.width, f.H = l.height, f.row_len = (uint32_t)L;
    f.first_band_chunk = l.first_band_chunk;
    f.filt = dec->filt.as<uint8_t>();
    f.slot_stride = (uint32_t)(((uint64_t)l.band_rows * L + SLOT_ALIGN - 1) / SLOT_ALIGN * SLOT_ALIGN);
    // every slot but the last is a whole stride; the last holds the rows that are left
    f.filt_bytes = (size_t)(l.n_bands - 1) * f.slot_stride + (size_t)(band_row_count(l, l.n_bands - 1) * L) + FILT_PAD;
    TF_REQUIRE(f.filt_bytes <= dec->filt_bytes && l.n_bands <= (uint32_t)dec->max_h, "tf_pngdec_decode_dev: %u bands of %u bytes: beyond the handle",
               l.n_bands, f.slot_stride); // (never: the frame is within the handle's size)
    memcpy(dec->stage.p, file, n);
    uint32_t *status = dec->status.as<uint32_t>();
    TF_HIP(hipMemcpyAsync(dec->file.p, dec->stage.p, n, hipMemcpyHostToDevice, stream()));
    TF_HIP(hipMemcpyAsync(dec->bands.p, dec->bands_host.p, 2 * (size_t)dec->max_h * sizeof(uint32_t), hipMemcpyHostToDevice, stream()));
    TF_HIP(hipMemsetAsync(dec->status.p, 0xFF, ST_WORDS * sizeof(uint32_t), stream()));
    TF_TRY(launch("pd_crc", k_pd_crc, dim3(l.n_bands), dim3(WAVE), 0, f, dec->dev_consts.as<Crc32Consts>(), status));
    TF_TRY(launch("pd_inflate", k_pd_inflate, dim3(l.n_bands), dim3(WAVE), 0, f, status));
    TF_TRY(launch("pd_rows", k_pd_rows, dim3(l.height), dim3(ROWS_BLOCK), 0, f, dec->rowsums.as<uint32_t>(), status));
    TF_TRY(launch("pd_unfilter", k_pd_unfilter, dim3(l.height), dim3(WAVE), 0, f, (uint8_t *)pix_dev, bgr, (const uint32_t *)status));
    TF_HIP(hipMemcpyAsync(dec->status_host.p, dec->status.p, ST_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipMemcpyAsync(dec->rowsums_host.p, dec->rowsums.p, 2 * (size_t)l.height * sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    const uint32_t *st = dec->status_host.as<uint32_t>();
    if (st[ST_CRC] != ST_NONE)
        return rejected(reject, make_reject(R_CHUNK_CRC, st[ST_CRC]));
    if (st[ST_BAND] != ST_NONE)
        return rejected(reject, make_reject(R_BAND + (st[ST_BAND] & 0xFFu), st[ST_BAND] >> 8));
    if (st[ST_FILTER] != ST_NONE)
        return rejected(reject, make_reject(R_FILTER_TYPE, st[ST_FILTER]));
    if (adler_of_rows(dec->rowsums_host.as<uint32_t>(), l.height, L) != l.adler)
        return rejected(reject, R_ADLER);
    return TF_OK;
}

TF_API int tf_pngdec_decode(tf_pngdec *dec, const uint8_t *file, size_t n, uint8_t *pix_host, int bgr, uint32_t *reject)
{
    TF_REQUIRE(dec && pix_host && reject, "tf_pngdec_decode: null pointer");
    if (!dec->out.p)
        TF_TRY(dec->out.alloc((size_t)dec->max_w * dec->max_h * 3 + 4));
    TF_TRY(tf_pngdec_decode_dev(dec, file, n, dec->out.p, bgr, reject));
    TF_HIP(hipMemcpyAsync(pix_host, dec->out.p, (size_t)dec->layout.width * dec->layout.height * 3, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}
