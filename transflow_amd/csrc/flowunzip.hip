// A flow archive member inflated where the flow is wanted (tests/flowunzip_ref.py is the Python
// statement of the same rules).  The member's stream is cut into bands by the index its writer left in the archive: band
// b is a byte range that inflates, on its own, to bytes [b B, min(N, (b + 1) B)) of S = the `.npy` header ‖ the array.
//
//   k_fu_inflate   one wave per band.  Lane 0 runs the machine of flowunzip_common.h -- the bit reader over a window of
//                  the band's compressed bytes in LDS, the block headers, the code tables in LDS, the literals -- and
//                  the wave does what the machine hands out: it refills the window with coalesced loads, copies a match
//                  or a stored block's bytes, and flushes.  The band's last 32768 bytes are a ring in LDS: a match reads
//                  the ring, never the destination, so no load of this kernel depends on a store of another lane to
//                  global memory; loads and stores of the ring by different lanes have a barrier between them.  The
//                  ring's new bytes go out as whole 64-byte lines, below `split` to the head buffer, from `split` on to
//                  the caller's array.  An archive is untrusted: every load is checked against the band's compressed
//                  range, every store against its output range, and a rejected band says why in its status word.
//   k_fu_crc       one wave per band, after the inflate kernel has ended: the lanes take contiguous slices of the band's
//                  bytes, the slices' CRC-32s are combined by x^(8 * bytes behind).
//   k_fu_finish    one work-group: the member's CRC-32 from the bands', the first rejected band.
//   k_fu_i64_f32   astype(float32) of int64 values.
#include "flowunzip_common.h"

#include "common.h"
#include "crc32_common.h"

namespace tf {
namespace flowunzip {

constexpr int WAVE = 64;
constexpr uint32_t MAX_SPLIT = 4096;
constexpr uint32_t NO_BAND = 0xFFFFFFFFu;

struct Member {
    const uint8_t *stream;   // the compressed bytes, stream_bytes of them
    const uint32_t *offsets; // n_bands + 1: where each band's range begins, and where the last ends
    uint32_t stream_bytes, band_bytes, usize, split;
    uint8_t *head; // MAX_SPLIT bytes: S below split
    uint8_t *data; // usize - split bytes: S from split on (4-byte aligned)
};

// ---- byte g of S goes to / comes from its place (g < usize: the callers check) ----------------------------------------------
__device__ __forceinline__ uint8_t *place(const Member &m, uint32_t g)
{
    return g < m.split ? m.head + g : m.data + (g - m.split);
}

// ---- inflate -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_fu_inflate(const Member m, uint32_t *__restrict__ status)
{
    __shared__ uint32_t s_ring[RING_BYTES / 4];
    __shared__ uint32_t s_win[WINDOW_BYTES / 4];
    __shared__ Code s_lit, s_dist;
    __shared__ uint32_t s_lengths[MAX_LENGTHS / 4];
    uint8_t *ring = reinterpret_cast<uint8_t *>(s_ring);
    uint8_t *win = reinterpret_cast<uint8_t *>(s_win);
    const int lane = threadIdx.x;
    const uint32_t band = blockIdx.x;
    const uint32_t first = band * m.band_bytes; // (n_bands * band_bytes < usize + band_bytes <= 2^31 + 2^28: the host checks)
    const uint32_t out_bytes = min(m.band_bytes, m.usize - first);
    const uint32_t off = m.offsets[band], end = m.offsets[band + 1];
    if (off > end || end > m.stream_bytes) { // (never: the host makes the offsets)
        if (lane == 0)
            status[band] = R_EXHAUSTED;
        return;
    }
    const uint32_t size = end - off;
    State s;
    start(s, win, size, out_bytes);
    for (;;) {
        Action x = make_action(A_DONE, R_OK, 0, 0);
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
                if (i < x.b && x.a + i < size)
                    v = m.stream[(size_t)off + x.a + i];
                if (i < x.b)
                    win[i] = v;
            }
        } else if (x.kind == A_MATCH) {
            const uint32_t at = x.a, len = x.b, d = x.c;
            if (d == 0 || d > at || d > RING_BYTES || len > 258 || len > out_bytes - min(at, out_bytes)) { // (never: step checked)
                if (lane == 0)
                    status[band] = R_DISTANCE;
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
                const bool mine = i < x.b && x.c + i < size && x.a + i < out_bytes;
                uint8_t v = 0;
                if (mine)
                    v = m.stream[(size_t)off + x.c + i];
                if (mine)
                    ring[(x.a + i) & RING_MASK] = v;
            }
        } else if (x.kind == A_FLUSH || (x.kind == A_DONE && x.a == R_OK)) {
            const uint32_t upto = x.kind == A_DONE ? produced : produced & ~63u; // flushed is a multiple of 64
            if (upto > out_bytes || upto - flushed > RING_BYTES || flushed > upto) { // (never)
                if (lane == 0)
                    status[band] = R_OVERRUN;
                return;
            }
            const uint32_t words_end = flushed + ((upto - flushed) & ~3u);
            for (uint32_t w = flushed + 4 * (uint32_t)lane; w < words_end; w += 4 * WAVE)
                if (w + 4 <= out_bytes) // split is a multiple of 64: a word lies on one side of it
                    *reinterpret_cast<uint32_t *>(place(m, first + w)) = s_ring[(w & RING_MASK) >> 2];
            for (uint32_t i = words_end + lane; i < upto; i += WAVE)
                if (i < out_bytes)
                    *place(m, first + i) = ring[i & RING_MASK];
            if (lane == 0)
                s.flushed = upto;
        }
        if (x.kind == A_DONE) {
            if (lane == 0)
                status[band] = x.a;
            return;
        }
        __syncthreads(); // the wave's bytes are in LDS before lane 0 goes on
    }
}

// ---- CRC-32 ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_fu_crc(const Member m, const Crc32Consts *__restrict__ consts, uint32_t *__restrict__ band_crc)
{
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_x2n[32];
    const int lane = threadIdx.x;
    crc32_stage_table(s_crc, consts, lane, WAVE);
    crc32_stage_x2n(s_x2n, consts, lane);
    __syncthreads();
    const uint32_t first = blockIdx.x * m.band_bytes;
    const uint32_t n = min(m.band_bytes, m.usize - first);
    const uint32_t slice = ((n + WAVE - 1) / WAVE + 3) & ~3u; // whole words: first and split are multiples of 64
    const uint32_t begin = min((uint32_t)lane * slice, n), end = min(begin + slice, n);
    uint32_t c = 0xFFFFFFFFu, j = begin;
    for (; j + 4 <= end; j += 4) {
        uint32_t v = *reinterpret_cast<const uint32_t *>(place(m, first + j));
#pragma unroll
        for (int k = 0; k < 4; k++, v >>= 8)
            c = crc32_update(c, v, s_crc);
    }
    for (; j < end; j++)
        c = crc32_update(c, *place(m, first + j), s_crc);
    c = crc32_wave_xor(crc32_shift(~c, n - end, s_x2n)); // ~c: the slice's own CRC-32 (of no bytes: 0)
    if (lane == 0)
        band_crc[blockIdx.x] = c;
}

constexpr int FINISH_BLOCK = 1024;
// info[0]: the CRC-32 of S, info[1]: the first rejected band (NO_BAND: none), info[2]: why
__global__ __launch_bounds__(FINISH_BLOCK) void k_fu_finish(const uint32_t *__restrict__ band_crc, const uint32_t *__restrict__ status,
                                                            uint32_t n_bands, uint32_t band_bytes, uint32_t usize,
                                                            const Crc32Consts *__restrict__ consts, uint32_t *__restrict__ info)
{
    __shared__ uint32_t s_x2n[32];
    __shared__ uint32_t s_crc, s_bad;
    const int tid = threadIdx.x;
    crc32_stage_x2n(s_x2n, consts, tid);
    if (tid == 0)
        s_crc = 0, s_bad = NO_BAND;
    __syncthreads();
    uint32_t crc = 0, bad = NO_BAND;
    for (uint32_t i = tid; i < n_bands; i += FINISH_BLOCK) {
        const unsigned long long end = min((unsigned long long)usize, ((unsigned long long)i + 1) * band_bytes);
        crc ^= crc32_shift(band_crc[i], usize - (uint32_t)end, s_x2n);
        if (status[i] != R_OK)
            bad = min(bad, i);
    }
    if (crc)
        atomicXor(&s_crc, crc);
    if (bad != NO_BAND)
        atomicMin(&s_bad, bad);
    __syncthreads();
    if (tid == 0) {
        info[0] = s_crc, info[1] = s_bad;
        info[2] = s_bad != NO_BAND ? status[s_bad] : 0;
    }
}

// ---- astype(float32) of int64 ------------------------------------------------------------------------------------------
constexpr int CONVERT_BLOCK = 256;
__global__ __launch_bounds__(CONVERT_BLOCK) void k_fu_i64_f32(const long long *__restrict__ in, size_t n, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * CONVERT_BLOCK + threadIdx.x;
    if (i < n)
        out[i] = (float)in[i]; // to nearest, ties to even: the conversion numpy's astype compiles to
}

} // namespace flowunzip
} // namespace tf

using namespace tf;
using namespace tf::flowunzip;

struct tf_flowunzip {
    size_t max_stream = 0, max_bands = 0;
    DevBuf consts, stream, offsets, status, band_crc, head, info, out;
    PinnedBuf offsets_host; // page-locked uint32_t: max_bands + 1
    PinnedBuf info_host;    // page-locked uint32_t: the CRC-32, the first rejected band, why
};

TF_API void tf_flowunzip_destroy(tf_flowunzip *h) { delete h; }

TF_API int tf_flowunzip_create(tf_flowunzip **out, size_t max_stream_bytes, size_t max_bands)
{
    TF_REQUIRE(out, "tf_flowunzip_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(max_stream_bytes >= 1 && max_stream_bytes <= ((size_t)1 << 31), "tf_flowunzip_create: a stream of %zu bytes (1 to 2^31)",
               max_stream_bytes);
    TF_REQUIRE(max_bands >= 1 && max_bands <= ((size_t)1 << 25), "tf_flowunzip_create: %zu bands (1 to 2^25)", max_bands);
    TF_TRY(ensure_init());
    auto h = make_handle<tf_flowunzip>();
    TF_REQUIRE(h, "tf_flowunzip_create: out of memory");
    h->max_stream = max_stream_bytes, h->max_bands = max_bands;
    Crc32Consts consts;
    make_crc32_consts(consts);
    TF_TRY(h->consts.alloc(sizeof(Crc32Consts)));
    TF_TRY(h->stream.alloc(max_stream_bytes));
    TF_TRY(h->offsets.alloc((max_bands + 1) * sizeof(uint32_t)));
    TF_TRY(h->status.alloc(max_bands * sizeof(uint32_t)));
    TF_TRY(h->band_crc.alloc(max_bands * sizeof(uint32_t)));
    TF_TRY(h->head.alloc(MAX_SPLIT));
    TF_TRY(h->info.alloc(4 * sizeof(uint32_t)));
    TF_TRY(h->offsets_host.alloc((max_bands + 1) * sizeof(uint32_t)));
    TF_TRY(h->info_host.alloc(4 * sizeof(uint32_t)));
    TF_HIP(hipMemcpyAsync(h->consts.p, &consts, sizeof(Crc32Consts), hipMemcpyHostToDevice, stream()));
    TF_HIP(hipStreamSynchronize(stream())); // `consts` is on this stack
    *out = h.release();
    return TF_OK;
}

TF_API int tf_flowunzip_decode_dev(tf_flowunzip *h, const uint8_t *stream_host, size_t stream_bytes, const uint32_t *band_sizes_host,
                                   size_t n_bands, size_t band_bytes, size_t usize, size_t split, uint8_t *head_out_host, void *data_dev,
                                   uint32_t *crc32, uint32_t *bad_band)
{
    TF_REQUIRE(h && stream_host && band_sizes_host && crc32 && bad_band && (head_out_host || split == 0), "tf_flowunzip_decode_dev: null pointer");
    *crc32 = 0, *bad_band = NO_BAND;
    TF_REQUIRE(split % 64 == 0 && split <= MAX_SPLIT, "tf_flowunzip_decode_dev: a split at %zu (a multiple of 64, at most %u)", split, MAX_SPLIT);
    TF_REQUIRE(band_bytes >= 64 && band_bytes % 64 == 0 && band_bytes <= ((size_t)1 << 28),
               "tf_flowunzip_decode_dev: band_bytes %zu (a multiple of 64 up to 2^28)", band_bytes);
    TF_REQUIRE(usize >= 1 && usize <= ((size_t)1 << 31) && split <= usize, "tf_flowunzip_decode_dev: %zu bytes, split at %zu (1 to 2^31)", usize,
               split);
    TF_REQUIRE(n_bands == (usize + band_bytes - 1) / band_bytes, "tf_flowunzip_decode_dev: %zu bands for %zu bytes in bands of %zu", n_bands,
               usize, band_bytes);
    TF_REQUIRE(n_bands <= h->max_bands && stream_bytes >= 1 && stream_bytes <= h->max_stream,
               "tf_flowunzip_decode_dev: %zu bands, a stream of %zu bytes; the handle is for %zu and %zu", n_bands, stream_bytes, h->max_bands,
               h->max_stream);
    TF_REQUIRE((data_dev && (uintptr_t)data_dev % 4 == 0) || usize == split, "tf_flowunzip_decode_dev: the destination is null or not 4-byte aligned");
    uint32_t *offsets_host = h->offsets_host.as<uint32_t>();
    size_t at = 0;
    for (size_t b = 0; b < n_bands; b++) {
        offsets_host[b] = (uint32_t)at;
        at += band_sizes_host[b];
        TF_REQUIRE(at <= stream_bytes, "tf_flowunzip_decode_dev: the bands' sizes pass the stream's %zu bytes at band %zu", stream_bytes, b);
    }
    offsets_host[n_bands] = (uint32_t)at;
    Member m;
    m.stream = h->stream.as<uint8_t>(), m.offsets = h->offsets.as<uint32_t>();
    m.stream_bytes = (uint32_t)stream_bytes, m.band_bytes = (uint32_t)band_bytes, m.usize = (uint32_t)usize, m.split = (uint32_t)split;
    m.head = h->head.as<uint8_t>(), m.data = (uint8_t *)data_dev;
    TF_HIP(hipMemcpyAsync(h->stream.p, stream_host, stream_bytes, hipMemcpyHostToDevice, stream()));
    TF_HIP(hipMemcpyAsync(h->offsets.p, h->offsets_host.p, (n_bands + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, stream()));
    TF_TRY(launch("fu_inflate", k_fu_inflate, dim3((unsigned)n_bands), dim3(WAVE), 0, m, h->status.as<uint32_t>()));
    TF_TRY(launch("fu_crc", k_fu_crc, dim3((unsigned)n_bands), dim3(WAVE), 0, m, h->consts.as<Crc32Consts>(), h->band_crc.as<uint32_t>()));
    TF_TRY(launch("fu_finish", k_fu_finish, dim3(1), dim3(FINISH_BLOCK), 0, h->band_crc.as<uint32_t>(), h->status.as<uint32_t>(),
                  (uint32_t)n_bands, (uint32_t)band_bytes, (uint32_t)usize, h->consts.as<Crc32Consts>(), h->info.as<uint32_t>()));
    TF_HIP(hipMemcpyAsync(h->info_host.p, h->info.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
    if (split)
        TF_HIP(hipMemcpyAsync(head_out_host, h->head.p, split, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    const uint32_t *info = h->info_host.as<uint32_t>();
    if (info[1] != NO_BAND) {
        *bad_band = info[1];
        return set_error(TF_ERR_STATE, "tf_flowunzip_decode_dev: band %u is no valid band (reason %u)", info[1], info[2]);
    }
    *crc32 = info[0];
    return TF_OK;
}

TF_API int tf_flowunzip_decode(tf_flowunzip *h, const uint8_t *stream_host, size_t stream_bytes, const uint32_t *band_sizes_host, size_t n_bands,
                               size_t band_bytes, size_t usize, size_t split, uint8_t *head_out_host, void *data_host, uint32_t *crc32,
                               uint32_t *bad_band)
{
    TF_REQUIRE(h && (data_host || usize == split), "tf_flowunzip_decode: null pointer");
    TF_REQUIRE(usize <= ((size_t)1 << 31) && split <= usize, "tf_flowunzip_decode: %zu bytes, split at %zu", usize, split);
    const size_t n = usize - split;
    if (h->out.bytes < n + 4) {
        h->out.release();
        TF_TRY(h->out.alloc(n + 4));
    }
    TF_TRY(tf_flowunzip_decode_dev(h, stream_host, stream_bytes, band_sizes_host, n_bands, band_bytes, usize, split, head_out_host, h->out.p,
                                   crc32, bad_band));
    if (n) {
        TF_HIP(hipMemcpyAsync(data_host, h->out.p, n, hipMemcpyDeviceToHost, stream()));
        TF_HIP(hipStreamSynchronize(stream()));
    }
    return TF_OK;
}

TF_API int tf_flow_i64_to_f32_dev(const void *src_dev, size_t n_values, void *dst_dev)
{
    TF_REQUIRE((src_dev && dst_dev) || n_values == 0, "tf_flow_i64_to_f32_dev: null pointer");
    TF_REQUIRE(n_values <= ((size_t)1 << 32), "tf_flow_i64_to_f32_dev: %zu values (at most 2^32)", n_values);
    if (n_values == 0)
        return TF_OK;
    TF_TRY(ensure_init());
    return launch("fu_i64_f32", k_fu_i64_f32, dim3(cdiv(n_values, CONVERT_BLOCK)), dim3(CONVERT_BLOCK), 0, (const long long *)src_dev, n_values,
                  (float *)dst_dev);
}
