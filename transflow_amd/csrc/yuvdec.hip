// Planar YUV frames turned back into RGB / BGR where the frame is wanted (tf_yuvdec_*): the way
// back of yuv.hip.  The planes of a Y4M or raw .yuv file -- yuv444p, yuv422p, yuv420p or nv12, BT.601 or BT.709, tv or pc
// range -- go up the link (1.5 to 3 bytes a pixel instead of the RGB frame's 3) and the pixels are made on the device.
//
//   k_yuv_rgb<LAYOUT, LINEAR>  a lane takes 8 adjacent pixels of the 1 or 2 rows of its chroma block row: two dwords of Y
//                  a row and a dword each of U and V (two each at 4:4:4, the pairs as two dwords for nv12) in, 24 bytes a
//                  row out.  A run is read as dwords where it is whole and begins on a dword, else as bytes at clamped
//                  indices; a row's 24 bytes are stored as six dwords where they are whole and begin on a dword, else as
//                  bytes.  LINEAR: the centre-sited triangle filter; the sample either side and, at 4:2:0, the chroma
//                  rows above and below come from memory at clamped indices.  No LDS, nothing shared by lanes.
#include "common.h"
#include "yuv_common.h"

#include <cstring>

namespace tf {
namespace yuv {

constexpr int PX = 8;                      // pixels of a row per lane
constexpr int BLOCK_X = 64, BLOCK_Y = 4; // a wave is 64 lanes side by side on one row group

__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__device__ __forceinline__ bool on_dword(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// N bytes from p into v[]: dwords where the lane has all N (n == N) and p is on a dword; else the bytes at the indices
// 0 .. n-1, the last one again for the missing ones (n >= 1): nothing past p[n-1] is read
template <int N> __device__ __forceinline__ void load_run(const uint8_t *p, int n, uint32_t (&v)[N])
{
    static_assert(N % 4 == 0, "a run is whole dwords");
    if (n == N && on_dword(p)) {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int w = 0; w < N / 4; w++) {
            const uint32_t d = s[w];
            v[4 * w] = d & 255, v[4 * w + 1] = (d >> 8) & 255, v[4 * w + 2] = (d >> 16) & 255, v[4 * w + 3] = d >> 24;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++)
            v[i] = p[min(i, n - 1)];
    }
}

// A lane's chroma samples of one chroma row, both planes: e[0] and e[NC + 1] are the neighbours either side (LINEAR
// only), e[1 .. NC] the lane's own; every index clamped to the row.
template <int LAYOUT, int NC, bool LINEAR>
__device__ __forceinline__ void load_chroma(const uint8_t *chroma, size_t cw, size_t ch, int row, int c0, int n_c, int (&u)[NC + 2],
                                            int (&v)[NC + 2])
{
    const int last = (int)cw - 1, left = max(c0 - 1, 0), right = min(c0 + NC, last);
    if (LAYOUT == NV12) {
        const uint8_t *p = chroma + (size_t)row * cw * 2;
        if (n_c == NC && on_dword(p + 2 * (size_t)c0)) {
            uint32_t uv[2 * NC];
            load_run(p + 2 * (size_t)c0, 2 * NC, uv);
#pragma unroll
            for (int i = 0; i < NC; i++)
                u[i + 1] = (int)uv[2 * i], v[i + 1] = (int)uv[2 * i + 1];
        } else { // the last pair again for the missing ones
#pragma unroll
            for (int i = 0; i < NC; i++) {
                const uint8_t *q = p + 2 * (size_t)(c0 + min(i, n_c - 1));
                u[i + 1] = q[0], v[i + 1] = q[1];
            }
        }
        if (LINEAR) {
            u[0] = p[2 * left], v[0] = p[2 * left + 1];
            u[NC + 1] = p[2 * right], v[NC + 1] = p[2 * right + 1];
        }
    } else {
        const uint8_t *pu = chroma + (size_t)row * cw, *pv = pu + cw * ch;
        uint32_t a[NC], b[NC];
        load_run(pu + c0, n_c, a);
        load_run(pv + c0, n_c, b);
#pragma unroll
        for (int i = 0; i < NC; i++)
            u[i + 1] = (int)a[i], v[i + 1] = (int)b[i];
        if (LINEAR) {
            u[0] = pu[left], v[0] = pv[left];
            u[NC + 1] = pu[right], v[NC + 1] = pv[right];
        }
    }
}

// planes: the frame_bytes(W, H, LAYOUT) bytes of the layout at any address; out: uint8 [H][W][3] at any address, R first
// (order 0) or B first (order 1).  Grid: x over the groups of 8 columns, y over the chroma rows (row pairs at 4:2:0 and
// nv12).
template <int LAYOUT, bool LINEAR>
__global__ __launch_bounds__(BLOCK_X *BLOCK_Y) void k_yuv_rgb(const uint8_t *__restrict__ planes, int W, int H, const InvCoef c,
                                                                int order, uint8_t *__restrict__ out)
{
    constexpr int BWL = bw_log2(LAYOUT), BHL = bh_log2(LAYOUT), BH = 1 << BHL;
    constexpr int NC = PX >> BWL;               // chroma samples of a lane, per plane
    constexpr bool LIN = LINEAR && BWL == 1;     // at 4:4:4 the two modes are the same thing
    const int g = blockIdx.x * BLOCK_X + threadIdx.x, cy = blockIdx.y * BLOCK_Y + threadIdx.y;
    const int x0 = g * PX, y0 = cy << BHL;
    if (x0 >= W || y0 >= H)
        return;
    const int n_px = min(PX, W - x0);           // an edge lane has fewer
    const int n_c = (n_px + (1 << BWL) - 1) >> BWL, c0 = g * NC;
    const size_t cw = ((size_t)W + (1 << BWL) - 1) >> BWL, ch = ((size_t)H + BH - 1) >> BHL;
    const uint8_t *chroma = planes + (size_t)W * H;
    int u[NC + 2], v[NC + 2];
    load_chroma<LAYOUT, NC, LIN>(chroma, cw, ch, cy, c0, n_c, u, v);
#pragma unroll
    for (int r = 0; r < BH; r++) {
        const int y = y0 + r;
        if (y >= H)
            break;
        int pu[PX], pv[PX];                    // the chroma at each pixel, less 128
        if (!LIN) {
#pragma unroll
            for (int k = 0; k < PX; k++)
                pu[k] = u[(k >> BWL) + 1] - 128, pv[k] = v[(k >> BWL) + 1] - 128;
        } else if (BHL == 0) {
#pragma unroll
            for (int k = 0; k < PX; k++) {
                const int i = (k >> 1) + 1, o = (k & 1) ? i + 1 : i - 1, add = (k & 1) ? 2 : 1;
                pu[k] = ((3 * u[i] + u[o] + add) >> 2) - 128, pv[k] = ((3 * v[i] + v[o] + add) >> 2) - 128;
            }
        } else {
            // the nearer chroma row three times, the farther once: the row above for an even y, below for an odd one
            const int other = r == 0 ? max(cy - 1, 0) : min(cy + 1, (int)ch - 1);
            int ou[NC + 2], ov[NC + 2];
            load_chroma<LAYOUT, NC, true>(chroma, cw, ch, other, c0, n_c, ou, ov);
#pragma unroll
            for (int i = 0; i < NC + 2; i++)
                ou[i] += 3 * u[i], ov[i] += 3 * v[i];
#pragma unroll
            for (int k = 0; k < PX; k++) {
                const int i = (k >> 1) + 1, o = (k & 1) ? i + 1 : i - 1, add = (k & 1) ? 7 : 8;
                pu[k] = ((3 * ou[i] + ou[o] + add) >> 4) - 128, pv[k] = ((3 * ov[i] + ov[o] + add) >> 4) - 128;
            }
        }
        uint32_t luma[PX];
        load_run(planes + (size_t)y * W + x0, n_px, luma);
        uint32_t px[3 * PX];
#pragma unroll
        for (int k = 0; k < PX; k++) {
            const int base = c.cy * ((int)luma[k] - c.y_off) + (1 << (FRAC_BITS - 1));
            const uint32_t red = clamp255((base + c.rv * pv[k]) >> FRAC_BITS);
            const uint32_t green = clamp255((base + c.gu * pu[k] + c.gv * pv[k]) >> FRAC_BITS);
            const uint32_t blue = clamp255((base + c.bu * pu[k]) >> FRAC_BITS);
            px[3 * k] = order ? blue : red, px[3 * k + 1] = green, px[3 * k + 2] = order ? red : blue;
        }
        uint8_t *dst = out + ((size_t)y * W + x0) * 3;
        if (n_px == PX && on_dword(dst)) {
            uint32_t *d = reinterpret_cast<uint32_t *>(dst);
#pragma unroll
            for (int w = 0; w < 3 * PX / 4; w++)
                d[w] = px[4 * w] | (px[4 * w + 1] << 8) | (px[4 * w + 2] << 16) | (px[4 * w + 3] << 24);
        } else {
#pragma unroll
            for (int i = 0; i < 3 * PX; i++)
                if (i < 3 * n_px)
                    dst[i] = (uint8_t)px[i];
        }
    }
}

template <int LAYOUT>
static int convert_back_as(const char *const (&names)[2], const uint8_t *planes, int W, int H, const InvCoef &c, int chroma, int order,
                           uint8_t *out, dim3 grid, dim3 block)
{
    if (chroma == LINEAR)
        return launch(names[1], k_yuv_rgb<LAYOUT, true>, grid, block, 0, planes, W, H, c, order, out);
    return launch(names[0], k_yuv_rgb<LAYOUT, false>, grid, block, 0, planes, W, H, c, order, out);
}

static int convert_back(const void *planes_dev, int W, int H, int layout, const InvCoef &c, int chroma, int order, void *out_dev)
{
    static const char *const n444[2] = {"yuvdec_444p", "yuvdec_444p_linear"}, *const n422[2] = {"yuvdec_422p", "yuvdec_422p_linear"},
                             *const n420[2] = {"yuvdec_420p", "yuvdec_420p_linear"}, *const nnv[2] = {"yuvdec_nv12", "yuvdec_nv12_linear"};
    const dim3 block(BLOCK_X, BLOCK_Y);
    const dim3 grid(cdiv(cdiv((size_t)W, PX), BLOCK_X), cdiv(chroma_height(H, layout), BLOCK_Y));
    const uint8_t *planes = (const uint8_t *)planes_dev;
    uint8_t *out = (uint8_t *)out_dev;
    switch (layout) {
    case YUV444P:
        return convert_back_as<YUV444P>(n444, planes, W, H, c, chroma, order, out, grid, block);
    case YUV422P:
        return convert_back_as<YUV422P>(n422, planes, W, H, c, chroma, order, out, grid, block);
    case YUV420P:
        return convert_back_as<YUV420P>(n420, planes, W, H, c, chroma, order, out, grid, block);
    default:
        return convert_back_as<NV12>(nnv, planes, W, H, c, chroma, order, out, grid, block);
    }
}

} // namespace yuv
} // namespace tf

using namespace tf;
using namespace tf::yuv;

struct tf_yuvdec {
    int max_w = 0, max_h = 0;
    size_t room = 0;       // tf_yuv_frame_bytes(max_w, max_h, yuv444p): no layout of a frame within the size takes more
    DevBuf planes;         // the frame that went up
    PinnedBuf stage;       // page-locked uint8_t: the frame on its way up
    Event uploaded;        // behind the last upload out of `stage`
    bool in_flight = false;
};

TF_API int tf_yuvdec_coefficients(int matrix, int range, int32_t out[5])
{
    TF_REQUIRE(out, "tf_yuvdec_coefficients: null pointer");
    InvCoef c;
    TF_REQUIRE(make_inv_coef(matrix, range, &c), "tf_yuvdec_coefficients: matrix %d (0: bt601, 1: bt709), range %d (0: tv, 1: pc)", matrix,
               range);
    out[0] = c.cy, out[1] = c.rv, out[2] = c.gu, out[3] = c.gv, out[4] = c.bu;
    return TF_OK;
}

TF_API void tf_yuvdec_destroy(tf_yuvdec *h)
{
    if (h && h->in_flight)
        (void)hipEventSynchronize(h->uploaded); // the link may still be reading the staging buffer
    delete h;
}

TF_API int tf_yuvdec_create(tf_yuvdec **out, int max_width, int max_height)
{
    TF_REQUIRE(out, "tf_yuvdec_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(max_height >= 1 && max_width >= 1 && max_height <= 65535 && max_width <= 65535, "tf_yuvdec_create: bad size %dx%d (1 to 65535)",
               max_width, max_height);
    TF_TRY(ensure_init());
    auto h = make_handle<tf_yuvdec>(tf_yuvdec_destroy);
    TF_REQUIRE(h, "tf_yuvdec_create: out of memory");
    h->max_w = max_width, h->max_h = max_height;
    h->room = frame_bytes(max_width, max_height, YUV444P);
    TF_TRY(h->planes.alloc(h->room));
    TF_TRY(h->stage.alloc(h->room));
    TF_TRY(h->uploaded.create());
    *out = h.release();
    return TF_OK;
}

// what both entry points check; the coefficients of the pair
static int yuvdec_args(const char *who, const tf_yuvdec *h, const void *planes, size_t nbytes, int width, int height, int layout, int matrix,
                       int range, int chroma, const void *out_dev, int order, InvCoef *c)
{
    TF_REQUIRE(h && planes && out_dev, "%s: null pointer", who);
    TF_REQUIRE(layout >= 0 && layout < N_LAYOUTS, "%s: layout %d (0: yuv444p, 1: yuv422p, 2: yuv420p, 3: nv12)", who, layout);
    TF_REQUIRE(make_inv_coef(matrix, range, c), "%s: matrix %d (0: bt601, 1: bt709), range %d (0: tv, 1: pc)", who, matrix, range);
    TF_REQUIRE(chroma >= 0 && chroma < N_CHROMAS, "%s: chroma %d (0: replicate, 1: linear)", who, chroma);
    TF_REQUIRE(order == 0 || order == 1, "%s: order %d (0: RGB, 1: BGR)", who, order);
    TF_REQUIRE(width >= 1 && height >= 1 && width <= h->max_w && height <= h->max_h, "%s: a frame of %dx%d; the handle is for %dx%d", who, width,
               height, h->max_w, h->max_h);
    TF_REQUIRE(nbytes == frame_bytes(width, height, layout), "%s: %zu bytes; a frame of %dx%d in layout %d has %zu", who, nbytes, width, height,
               layout, frame_bytes(width, height, layout));
    return TF_OK;
}

TF_API int tf_yuvdec_convert_dev(tf_yuvdec *h, const void *planes_dev, size_t nbytes, int width, int height, int layout, int matrix, int range,
                                 int chroma, void *out_dev, int order)
{
    InvCoef c;
    TF_TRY(yuvdec_args("tf_yuvdec_convert_dev", h, planes_dev, nbytes, width, height, layout, matrix, range, chroma, out_dev, order, &c));
    return convert_back(planes_dev, width, height, layout, c, chroma, order, out_dev);
}

TF_API int tf_yuvdec_convert(tf_yuvdec *h, const uint8_t *planes_host, size_t nbytes, int width, int height, int layout, int matrix, int range,
                             int chroma, void *out_dev, int order)
{
    InvCoef c;
    TF_TRY(yuvdec_args("tf_yuvdec_convert", h, planes_host, nbytes, width, height, layout, matrix, range, chroma, out_dev, order, &c));
    if (h->in_flight) { // the staging buffer is written again only when the link has read it
        TF_HIP(hipEventSynchronize(h->uploaded));
        h->in_flight = false;
    }
    memcpy(h->stage.p, planes_host, nbytes);
    // (an earlier call's kernel may still read h->planes: on the same stream the copy queues behind it; a caller that
    // changes streams between calls orders them itself, as with every handle)
    TF_HIP(hipMemcpyAsync(h->planes.p, h->stage.p, nbytes, hipMemcpyHostToDevice, stream()));
    TF_HIP(hipEventRecord(h->uploaded, stream()));
    h->in_flight = true;
    return convert_back(h->planes.p, width, height, layout, c, chroma, order, out_dev);
}
