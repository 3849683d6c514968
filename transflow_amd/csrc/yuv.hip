// Planar YUV of a frame that is in device memory (tf_yuv_*): the layout a video encoder takes --
// yuv444p, yuv422p, yuv420p or nv12, BT.601 or BT.709, tv or pc range -- made where the frame is, so that 1.5 to 3 bytes
// a pixel come down instead of the RGB frame's 3 and nobody converts on the host.
//
//   k_yuv<LAYOUT>  a lane takes 8 adjacent pixels of the 1 or 2 rows of its chroma blocks: 24 bytes a row in, two dwords
//                  of Y a row and a dword each of U and V (two each at 4:4:4, the pair as U V U V for nv12) out.  A row is
//                  read as dwords where its bytes of the lane begin on a dword, else as bytes; a run of samples is stored
//                  as dwords where it is whole and begins on a dword, else as bytes.  No LDS, nothing shared by lanes.
#include "common.h"
#include "yuv_common.h"

#include <cstring>

namespace tf {
namespace yuv {

constexpr int PX = 8;                   // pixels of a row per lane
constexpr int BLOCK_X = 64, BLOCK_Y = 4; // a wave is 64 lanes side by side on one row group

__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__device__ __forceinline__ bool on_dword(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// n of the N samples v[] to dst: dwords for a whole run that begins on a dword, bytes for an edge lane's and any other
template <int N> __device__ __forceinline__ void store_run(uint8_t *dst, const uint32_t (&v)[N], int n)
{
    static_assert(N % 4 == 0, "a run is whole dwords");
    if (n == N && on_dword(dst)) {
        uint32_t *d = reinterpret_cast<uint32_t *>(dst);
#pragma unroll
        for (int w = 0; w < N / 4; w++)
            d[w] = v[4 * w] | (v[4 * w + 1] << 8) | (v[4 * w + 2] << 16) | (v[4 * w + 3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < N; i++)
            if (i < n)
                dst[i] = (uint8_t)v[i];
    }
}

// rgb: uint8 [H][W][3] at any address; out: the frame_bytes(W, H, LAYOUT) bytes of the layout at any address.
// Grid: x over the groups of 8 columns, y over the chroma rows (row pairs at 4:2:0 and nv12).
template <int LAYOUT>
__global__ __launch_bounds__(BLOCK_X *BLOCK_Y) void k_yuv(const uint8_t *__restrict__ rgb, int W, int H, const Coef c,
                                                          uint8_t *__restrict__ out)
{
    constexpr int BWL = bw_log2(LAYOUT), BHL = bh_log2(LAYOUT), BH = 1 << BHL, K = BWL + BHL;
    constexpr int NC = PX >> BWL; // chroma samples of a lane, per plane
    const int g = blockIdx.x * BLOCK_X + threadIdx.x, cy = blockIdx.y * BLOCK_Y + threadIdx.y;
    const int x0 = g * PX, y0 = cy << BHL;
    if (x0 >= W || y0 >= H)
        return;
    const int n_px = min(PX, W - x0); // an edge lane has fewer: its last pixel stands for the missing ones
    int sr[NC], sg[NC], sb[NC];
#pragma unroll
    for (int i = 0; i < NC; i++)
        sr[i] = sg[i] = sb[i] = 0;
#pragma unroll
    for (int r = 0; r < BH; r++) {
        const int y = min(y0 + r, H - 1); // below an odd height the last row again
        const uint8_t *src = rgb + ((size_t)y * W + x0) * 3;
        uint32_t px[3 * PX];
        if (n_px == PX && on_dword(src)) {
            const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
#pragma unroll
            for (int w = 0; w < 3 * PX / 4; w++) {
                const uint32_t d = s[w];
                px[4 * w] = d & 255, px[4 * w + 1] = (d >> 8) & 255, px[4 * w + 2] = (d >> 16) & 255, px[4 * w + 3] = d >> 24;
            }
        } else {
#pragma unroll
            for (int k = 0; k < PX; k++) {
                const uint8_t *p = src + 3 * min(k, n_px - 1);
                px[3 * k] = p[0], px[3 * k + 1] = p[1], px[3 * k + 2] = p[2];
            }
        }
        if (y0 + r < H) {
            uint32_t luma[PX];
#pragma unroll
            for (int k = 0; k < PX; k++)
                luma[k] = clamp255((c.y[0] * (int)px[3 * k] + c.y[1] * (int)px[3 * k + 1] + c.y[2] * (int)px[3 * k + 2] + c.y_add) >>
                                   FRAC_BITS);
            store_run(out + (size_t)y * W + x0, luma, n_px);
        }
#pragma unroll
        for (int k = 0; k < PX; k++)
            sr[k >> BWL] += (int)px[3 * k], sg[k >> BWL] += (int)px[3 * k + 1], sb[k >> BWL] += (int)px[3 * k + 2];
    }
    // the mean of the block's unrounded values, rounded once: 128.5 in the units of the sum of 2^K pixels
    constexpr int C_ADD = (128 << (FRAC_BITS + K)) + (1 << (FRAC_BITS - 1 + K));
    uint32_t u[NC], v[NC];
#pragma unroll
    for (int i = 0; i < NC; i++) {
        u[i] = clamp255((c.u[0] * sr[i] + c.u[1] * sg[i] + c.u[2] * sb[i] + C_ADD) >> (FRAC_BITS + K));
        v[i] = clamp255((c.v[0] * sr[i] + c.v[1] * sg[i] + c.v[2] * sb[i] + C_ADD) >> (FRAC_BITS + K));
    }
    const int n_c = (n_px + (1 << BWL) - 1) >> BWL;
    const size_t cw = ((size_t)W + (1 << BWL) - 1) >> BWL, ch = ((size_t)H + BH - 1) >> BHL;
    uint8_t *chroma = out + (size_t)W * H;
    if (LAYOUT == NV12) {
        uint32_t uv[2 * NC];
#pragma unroll
        for (int i = 0; i < NC; i++)
            uv[2 * i] = u[i], uv[2 * i + 1] = v[i];
        store_run(chroma + ((size_t)cy * cw + (size_t)g * NC) * 2, uv, 2 * n_c);
    } else {
        const size_t at = (size_t)cy * cw + (size_t)g * NC;
        store_run(chroma + at, u, n_c);
        store_run(chroma + cw * ch + at, v, n_c);
    }
}

static int convert(const void *rgb_dev, int W, int H, int layout, const Coef &c, void *out_dev)
{
    const dim3 block(BLOCK_X, BLOCK_Y);
    const dim3 grid(cdiv(cdiv((size_t)W, PX), BLOCK_X), cdiv(chroma_height(H, layout), BLOCK_Y));
    const uint8_t *rgb = (const uint8_t *)rgb_dev;
    uint8_t *out = (uint8_t *)out_dev;
    switch (layout) {
    case YUV444P:
        return launch("yuv_444p", k_yuv<YUV444P>, grid, block, 0, rgb, W, H, c, out);
    case YUV422P:
        return launch("yuv_422p", k_yuv<YUV422P>, grid, block, 0, rgb, W, H, c, out);
    case YUV420P:
        return launch("yuv_420p", k_yuv<YUV420P>, grid, block, 0, rgb, W, H, c, out);
    default:
        return launch("yuv_nv12", k_yuv<NV12>, grid, block, 0, rgb, W, H, c, out);
    }
}

// whether a host address is page-locked memory the runtime knows (tf_host_alloc's): a copy to it needs no staging
static bool page_locked(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); // an address the runtime has never seen is an error to it, not to the caller
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

} // namespace yuv
} // namespace tf

using namespace tf;
using namespace tf::yuv;

struct tf_yuv {
    int H = 0, W = 0, layout = 0;
    Coef coef;
    size_t bytes = 0;
    DevBuf out, upload;
    PinnedBuf host; // page-locked uint8_t: the planes on their way to a caller's pageable buffer
};

TF_API size_t tf_yuv_frame_bytes(int width, int height, int layout) { return frame_bytes(width, height, layout); }

TF_API int tf_yuv_coefficients(int matrix, int range, int32_t out[9], int32_t *y_offset)
{
    TF_REQUIRE(out && y_offset, "tf_yuv_coefficients: null pointer");
    Coef c;
    TF_REQUIRE(make_coef(matrix, range, &c), "tf_yuv_coefficients: matrix %d (0: bt601, 1: bt709), range %d (0: tv, 1: pc)", matrix, range);
    for (int i = 0; i < 3; i++)
        out[i] = c.y[i], out[3 + i] = c.u[i], out[6 + i] = c.v[i];
    *y_offset = c.y_add >> FRAC_BITS;
    return TF_OK;
}

TF_API void tf_yuv_destroy(tf_yuv *h) { delete h; }

TF_API int tf_yuv_create(tf_yuv **out, int height, int width, int layout, int matrix, int range)
{
    TF_REQUIRE(out, "tf_yuv_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(height >= 1 && width >= 1 && height <= 65535 && width <= 65535, "tf_yuv_create: bad size %dx%d (1 to 65535)", width,
               height);
    TF_REQUIRE(layout >= 0 && layout < N_LAYOUTS, "tf_yuv_create: layout %d (0: yuv444p, 1: yuv422p, 2: yuv420p, 3: nv12)", layout);
    Coef c;
    TF_REQUIRE(make_coef(matrix, range, &c), "tf_yuv_create: matrix %d (0: bt601, 1: bt709), range %d (0: tv, 1: pc)", matrix, range);
    TF_TRY(ensure_init());
    auto h = make_handle<tf_yuv>();
    TF_REQUIRE(h, "tf_yuv_create: out of memory");
    h->H = height, h->W = width, h->layout = layout, h->coef = c;
    h->bytes = frame_bytes(width, height, layout);
    TF_TRY(h->out.alloc(h->bytes));
    TF_TRY(h->host.alloc(h->bytes));
    *out = h.release();
    return TF_OK;
}

TF_API int tf_yuv_convert_to_dev(tf_yuv *h, const void *rgb_dev, void *out_dev)
{
    TF_REQUIRE(h && rgb_dev && out_dev, "tf_yuv_convert_to_dev: null pointer");
    return convert(rgb_dev, h->W, h->H, h->layout, h->coef, out_dev);
}

TF_API int tf_yuv_convert_dev(tf_yuv *h, const void *rgb_dev, uint8_t *out_host, size_t capacity, size_t *n_bytes)
{
    TF_REQUIRE(h && rgb_dev && n_bytes && (out_host || capacity == 0), "tf_yuv_convert_dev: null pointer");
    *n_bytes = h->bytes;
    TF_REQUIRE(h->bytes <= capacity, "tf_yuv_convert_dev: the frame has %zu bytes, the buffer %zu", h->bytes, capacity);
    TF_TRY(convert(rgb_dev, h->W, h->H, h->layout, h->coef, h->out.p));
    // straight into the caller's buffer where the link can write it; else by way of the handle's page-locked one
    void *down = page_locked(out_host) ? (void *)out_host : h->host.p;
    TF_HIP(hipMemcpyAsync(down, h->out.p, h->bytes, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    if (down != out_host)
        memcpy(out_host, down, h->bytes);
    return TF_OK;
}

TF_API int tf_yuv_convert(tf_yuv *h, const uint8_t *rgb_host, uint8_t *out_host, size_t capacity, size_t *n_bytes)
{
    TF_REQUIRE(h && rgb_host && n_bytes && (out_host || capacity == 0), "tf_yuv_convert: null pointer");
    *n_bytes = h->bytes;
    TF_REQUIRE(h->bytes <= capacity, "tf_yuv_convert: the frame has %zu bytes, the buffer %zu", h->bytes, capacity);
    TF_TRY(h->upload.upload(rgb_host, (size_t)h->H * h->W * 3));
    return tf_yuv_convert_dev(h, h->upload.p, out_host, capacity, n_bytes);
}
