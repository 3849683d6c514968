// Lucas-Kanade: calc_optical_flow_lukas_kanade (transflow/flow/methods/lukas_kanade.py) on the GPU, the float32 flow
// of cv2.calcOpticalFlowPyrLK over a grid of points, as tests/lk_ref.py restates OpenCV 4.x's lkpyramid.cpp.
//
//   k_lk_pad0     level 0 of a frame's pyramid: the frame copied into a buffer padded by win, reflect-101
//   k_lk_pyrdown  level l from level l-1 (pyrDown), padded the same way
//   k_lk_scharr   calcSharrDeriv of a prev level, with a zero border of win
//   k_lk_track    one lane per point: every level, from the coarsest down, in registers, in one launch for n pairs;
//                 stores p1 - p0 into the step x step block of the point (the reference's kron and crop)
//
// Pyramids and derivatives belong to frame slots and carry the (win, levels) they were built for, so a frame that was
// "next" is not rebuilt when it becomes "prev".
#include "lk_common.h"

#include <cstring>
#include <memory>

namespace tf {
namespace lk {

__global__ void k_lk_pad0(const uint8_t *__restrict__ src, int W, int H, uint8_t *__restrict__ dst, Level lv, int P)
{
    const int px = blockIdx.x * blockDim.x + threadIdx.x, py = blockIdx.y;
    if (px >= lv.stride)
        return;
    const int x = reflect101(px - P, W), y = reflect101(py - P, H);
    dst[lv.origin + (long long)(py - P) * lv.stride + (px - P)] = src[(size_t)y * W + x];
}

// pyrDown: 5x5 [1 4 6 4 1]^2, (s + 128) >> 8, reflect-101 over the source level's own size (the sum is exact)
__global__ void k_lk_pyrdown(uint8_t *__restrict__ pyr, Level s, Level d, int P)
{
    const int px = blockIdx.x * blockDim.x + threadIdx.x, py = blockIdx.y;
    if (px >= d.stride)
        return;
    const int x = reflect101(px - P, d.w), y = reflect101(py - P, d.h);
    const int k[5] = {1, 4, 6, 4, 1};
    int cols[5];
#pragma unroll
    for (int j = 0; j < 5; j++)
        cols[j] = reflect101(2 * x + j - 2, s.w);
    int acc = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const uint8_t *row = pyr + s.origin + (long long)reflect101(2 * y + i - 2, s.h) * s.stride;
        int t = 0;
#pragma unroll
        for (int j = 0; j < 5; j++)
            t += k[j] * row[cols[j]];
        acc += k[i] * t;
    }
    pyr[d.origin + (long long)(py - P) * d.stride + (px - P)] = (uint8_t)((acc + 128) >> 8);
}

// calcSharrDeriv of one level into the padded derivative buffer; the pad is zero
__global__ void k_lk_scharr(const uint8_t *__restrict__ pyr, short2 *__restrict__ der, Level lv, int P)
{
    const int px = blockIdx.x * blockDim.x + threadIdx.x, py = blockIdx.y;
    if (px >= lv.stride)
        return;
    const int x = px - P, y = py - P;
    short2 out = make_short2(0, 0);
    if (x >= 0 && x < lv.w && y >= 0 && y < lv.h) {
        const uint8_t *img = pyr + lv.origin;
        const int ym = reflect101(y - 1, lv.h), yp = reflect101(y + 1, lv.h);
        const int xm = reflect101(x - 1, lv.w), xp = reflect101(x + 1, lv.w);
        int t0[3], t1[3];
        const int xs[3] = {xm, x, xp};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int r0 = img[(long long)ym * lv.stride + xs[c]], r1 = img[(long long)y * lv.stride + xs[c]],
                      r2 = img[(long long)yp * lv.stride + xs[c]];
            t0[c] = (r0 + r2) * 3 + r1 * 10;
            t1[c] = r2 - r0;
        }
        out = make_short2((short)(t0[2] - t0[0]), (short)((t1[2] + t1[0]) * 3 + t1[1] * 10));
    }
    der[lv.origin + (long long)y * lv.stride + x] = out;
}

// 14-bit bilinear weights: cvRound (half to even) of the float products
__device__ __forceinline__ void weights(float a, float b, int &w00, int &w01, int &w10, int &w11)
{
    const float s = (float)(1 << W_BITS);
    w00 = (int)rintf((1.f - a) * (1.f - b) * s);
    w01 = (int)rintf(a * (1.f - b) * s);
    w10 = (int)rintf((1.f - a) * b * s);
    w11 = (1 << W_BITS) - w00 - w01 - w10;
}

struct Bil {
    int w00, w01, w10, w11;
    __device__ __forceinline__ int u8(const uint8_t *p, int stride, int shift) const
    {
        const int s = p[0] * w00 + p[1] * w01 + p[stride] * w10 + p[stride + 1] * w11;
        return (s + (1 << (shift - 1))) >> shift;
    }
    __device__ __forceinline__ void d2(const short2 *p, int stride, int &gx, int &gy) const
    {
        const short2 a = p[0], b = p[1], c = p[stride], d = p[stride + 1];
        gx = (a.x * w00 + b.x * w01 + c.x * w10 + d.x * w11 + (1 << (W_BITS - 1))) >> W_BITS;
        gy = (a.y * w00 + b.y * w01 + c.y * w10 + d.y * w11 + (1 << (W_BITS - 1))) >> W_BITS;
    }
};

// The prev patch at window pixel (y, x): the I value x32 and the two derivatives.  `whole`: the weights are
// (2^14, 0, 0, 0), when the values are the pixel's own (x32 and as they are).
__device__ __forceinline__ void prev_px(const uint8_t *I, const short2 *D, int stride, const Bil &w, bool whole, int off,
                                        int &iv, int &gx, int &gy)
{
    if (whole) {
        iv = (int)I[off] << 5;
        const short2 d = D[off];
        gx = d.x, gy = d.y;
    } else {
        iv = w.u8(I + off, stride, W_BITS - 5);
        w.d2(D + off, stride, gx, gy);
    }
}

// LKTrackerInvoker::operator() for one point over levels L..0.  Returns nextPts.  The steps run at each level go to
// the block's counters s_sum / s_max (when given) and, with TRACE, {nextPts, steps, code} to trace[level].
template <bool TRACE>
__device__ float2 track_point(const Geometry &g, const uint8_t *Ib, const uint8_t *Jb, const short2 *Db, float p0x,
                              float p0y, unsigned *s_sum, unsigned *s_max, float4 *trace)
{
    const int win = g.win;
    const float half = (float)(win - 1) * 0.5f;
    float nx = p0x, ny = p0y; // nextPts[ptidx]
    for (int L = g.L; L >= 0; L--) {
        const Level lv = g.lv[L];
        const float scale = ldexpf(1.f, -L); // (float)(1./(1 << level)), exact
        float ppx = p0x * scale, ppy = p0y * scale;
        float cx, cy;
        if (L == g.L)
            cx = ppx, cy = ppy;
        else
            cx = nx * 2.f, cy = ny * 2.f;
        nx = cx, ny = cy;
        int its = 0, code = TR_DONE;
        ppx -= half, ppy -= half;
        const float fpx = floorf(ppx), fpy = floorf(ppy);
        if (!(fpx >= (float)-win && fpx < (float)lv.w && fpy >= (float)-win && fpy < (float)lv.h)) {
            code = TR_LOST_PREV;
        } else {
            const int ipx = (int)fpx, ipy = (int)fpy;
            Bil pw;
            weights(ppx - (float)ipx, ppy - (float)ipy, pw.w00, pw.w01, pw.w10, pw.w11);
            const bool whole = pw.w00 == (1 << W_BITS) && pw.w01 == 0 && pw.w10 == 0 && pw.w11 == 0;
            const long long pbase = lv.origin + (long long)ipy * lv.stride + ipx;
            const uint8_t *I = Ib + pbase;
            const short2 *D = Db + pbase;
            const int st = lv.stride;
            // A: four lane partials over the first 4 * (win / 4) columns, a scalar accumulator for the rest
            float q11[4] = {0.f, 0.f, 0.f, 0.f}, q12[4] = {0.f, 0.f, 0.f, 0.f}, q22[4] = {0.f, 0.f, 0.f, 0.f};
            float t11 = 0.f, t12 = 0.f, t22 = 0.f;
            for (int y = 0; y < win; y++) {
                int x = 0;
                for (; x <= win - 4; x += 4) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        int iv, gx, gy;
                        prev_px(I, D, st, pw, whole, y * st + x + k, iv, gx, gy);
                        const float fx = (float)gx, fy = (float)gy;
                        q22[k] = q22[k] + fy * fy;
                        q12[k] = q12[k] + fx * fy;
                        q11[k] = q11[k] + fx * fx;
                    }
                }
                for (; x < win; x++) {
                    int iv, gx, gy;
                    prev_px(I, D, st, pw, whole, y * st + x, iv, gx, gy);
                    t11 = t11 + (float)(gx * gx);
                    t12 = t12 + (float)(gx * gy);
                    t22 = t22 + (float)(gy * gy);
                }
            }
            const float FLT_SCALE = 1.f / (1 << 20);
            const float A11 = (t11 + ((q11[0] + q11[2]) + (q11[1] + q11[3]))) * FLT_SCALE;
            const float A12 = (t12 + ((q12[0] + q12[2]) + (q12[1] + q12[3]))) * FLT_SCALE;
            const float A22 = (t22 + ((q22[0] + q22[2]) + (q22[1] + q22[3]))) * FLT_SCALE;
            float Dt = A11 * A22 - A12 * A12;
            const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * win * win);
            if (minEig < 1e-4f || Dt < 1.19209290e-07f) {
                code = TR_LOST_EIG;
            } else {
                Dt = 1.f / Dt;
                cx -= half, cy -= half;
                float pdx = 0.f, pdy = 0.f;
                for (int j = 0; j < MAX_COUNT; j++) {
                    const float fnx = floorf(cx), fny = floorf(cy);
                    if (!(fnx >= (float)-win && fnx < (float)lv.w && fny >= (float)-win && fny < (float)lv.h)) {
                        code = TR_LOST_NEXT;
                        break;
                    }
                    const int inx = (int)fnx, iny = (int)fny;
                    Bil nw;
                    weights(cx - (float)inx, cy - (float)iny, nw.w00, nw.w01, nw.w10, nw.w11);
                    const uint8_t *J = Jb + lv.origin + (long long)iny * st + inx;
                    // b: per 8-column chunk, int32 pair dot products into two 4-lane partials; the rest into scalars
                    float qb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    float tb1 = 0.f, tb2 = 0.f;
                    for (int y = 0; y < win; y++) {
                        int x = 0;
                        for (; x <= win - 8; x += 8) {
                            int df[8], gxs[8], gys[8];
#pragma unroll
                            for (int k = 0; k < 8; k++) {
                                int iv;
                                prev_px(I, D, st, pw, whole, y * st + x + k, iv, gxs[k], gys[k]);
                                df[k] = nw.u8(J + y * st + x + k, st, W_BITS - 5) - iv;
                            }
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const int lane = (k >> 1) * 4 + (k & 1) * 2;
                                qb[lane] = qb[lane] + (float)(df[k] * gxs[k] + df[k + 4] * gxs[k + 4]);
                                qb[lane + 1] = qb[lane + 1] + (float)(df[k] * gys[k] + df[k + 4] * gys[k + 4]);
                            }
                        }
                        for (; x < win; x++) {
                            int iv, gx, gy;
                            prev_px(I, D, st, pw, whole, y * st + x, iv, gx, gy);
                            const int df = nw.u8(J + y * st + x, st, W_BITS - 5) - iv;
                            tb1 = tb1 + (float)(df * gx);
                            tb2 = tb2 + (float)(df * gy);
                        }
                    }
                    const float s0 = qb[0] + qb[4], s1 = qb[1] + qb[5], s2 = qb[2] + qb[6], s3 = qb[3] + qb[7];
                    const float b1 = (tb1 + (s0 + s2)) * FLT_SCALE, b2 = (tb2 + (s1 + s3)) * FLT_SCALE;
                    const float ddx = (A12 * b2 - A22 * b1) * Dt, ddy = (A12 * b1 - A11 * b2) * Dt;
                    cx += ddx, cy += ddy;
                    nx = cx + half, ny = cy + half;
                    its = j + 1;
                    if ((double)ddx * ddx + (double)ddy * ddy <= EPS2)
                        break;
                    if (j > 0 && (double)fabsf(ddx + pdx) < 0.01 && (double)fabsf(ddy + pdy) < 0.01) {
                        nx -= ddx * 0.5f, ny -= ddy * 0.5f;
                        break;
                    }
                    pdx = ddx, pdy = ddy;
                }
            }
        }
        if (s_sum) {
            atomicAdd(&s_sum[L], (unsigned)its);
            atomicMax(&s_max[L], (unsigned)its);
        }
        if (TRACE)
            trace[L] = make_float4(nx, ny, (float)its, (float)code);
    }
    return make_float2(nx, ny);
}

struct TrackOut {
    float2 *flow[MAX_PAIRS];
    unsigned long long *stats;      // [n_pairs][MAX_LEVELS][2] {sum, max} of steps per point, or null
};

__global__ void __launch_bounds__(TRACK_BX) k_lk_track(Geometry g, PairPtrs pp, TrackOut out, int W, int H, int step,
                                                       int gw, int npts)
{
    const int pair = blockIdx.y;
    const int t = blockIdx.x * TRACK_BX + threadIdx.x;
    __shared__ unsigned s_sum[MAX_LEVELS], s_max[MAX_LEVELS];
    const bool stats = out.stats != nullptr;
    if (stats) {
        if (threadIdx.x < MAX_LEVELS)
            s_sum[threadIdx.x] = 0, s_max[threadIdx.x] = 0;
        __syncthreads();
    }
    if (t < npts) {
        const int gi = t / gw, gj = t - gi * gw;
        const float p0x = (float)(gj * step), p0y = (float)(gi * step);
        const float2 p1 = track_point<false>(g, pp.I[pair], pp.J[pair], pp.D[pair], p0x, p0y, stats ? s_sum : nullptr,
                                             stats ? s_max : nullptr, nullptr);
        const float2 f = make_float2(p1.x - p0x, p1.y - p0y);
        float2 *dst = out.flow[pair];
        const int y0 = gi * step, x0 = gj * step;
        const int y1 = min(y0 + step, H), x1 = min(x0 + step, W);
        for (int y = y0; y < y1; y++)
            for (int x = x0; x < x1; x++)
                dst[(size_t)y * W + x] = f;
    }
    if (stats) {
        __syncthreads();
        if ((int)threadIdx.x <= g.L) {
            unsigned long long *s = out.stats + ((size_t)pair * MAX_LEVELS + threadIdx.x) * 2;
            atomicAdd(&s[0], (unsigned long long)s_sum[threadIdx.x]);
            atomicMax(&s[1], (unsigned long long)s_max[threadIdx.x]);
        }
    }
}

__global__ void k_lk_trace(Geometry g, const uint8_t *I, const uint8_t *J, const short2 *D, float px, float py,
                           float4 *trace)
{
    if (threadIdx.x == 0 && blockIdx.x == 0)
        (void)track_point<true>(g, I, J, D, px, py, nullptr, nullptr, trace);
}

} // namespace lk
} // namespace tf

using namespace tf;
using namespace tf::lk;

struct tf_lk {
    struct Slot {
        DevBuf pyr, der;
        int pyr_win = -1, pyr_L = -1, der_win = -1, der_L = -1;
    };
    int W = 0, H = 0, n_slots = 0, max_pairs = 0, last_pairs = 0, last_L = -1;
    DevBuf frames, flow, stats, bgr_stage;
    std::unique_ptr<Slot[]> slots;
    std::vector<unsigned long long> host_stats;
};

namespace {

int ensure_pyramid(tf_lk *lk, int slot, const Geometry &g)
{
    tf_lk::Slot &s = lk->slots[slot];
    if (s.pyr_win == g.win && s.pyr_L == g.L)
        return TF_OK;
    if (s.pyr.bytes < (size_t)g.elems)
        TF_TRY(s.pyr.alloc((size_t)g.elems));
    s.pyr_win = s.pyr_L = s.der_win = s.der_L = -1;
    uint8_t *pyr = s.pyr.as<uint8_t>();
    const uint8_t *src = lk->frames.as<uint8_t>() + (size_t)slot * lk->W * lk->H;
    const Level &l0 = g.lv[0];
    TF_TRY(launch("lk_pad0", k_lk_pad0, dim3(cdiv(l0.stride, 256), l0.h + 2 * g.P), dim3(256), 0, src, lk->W, lk->H, pyr,
                  l0, g.P));
    for (int l = 1; l <= g.L; l++) {
        const Level &d = g.lv[l];
        TF_TRY(launch("lk_pyrdown", k_lk_pyrdown, dim3(cdiv(d.stride, 256), d.h + 2 * g.P), dim3(256), 0, pyr, g.lv[l - 1],
                      d, g.P));
    }
    s.pyr_win = g.win, s.pyr_L = g.L;
    return TF_OK;
}

int ensure_derivs(tf_lk *lk, int slot, const Geometry &g)
{
    TF_TRY(ensure_pyramid(lk, slot, g));
    tf_lk::Slot &s = lk->slots[slot];
    if (s.der_win == g.win && s.der_L == g.L)
        return TF_OK;
    if (s.der.bytes < (size_t)g.elems * sizeof(short2))
        TF_TRY(s.der.alloc((size_t)g.elems * sizeof(short2)));
    for (int l = 0; l <= g.L; l++) {
        const Level &v = g.lv[l];
        TF_TRY(launch("lk_scharr", k_lk_scharr, dim3(cdiv(v.stride, 256), v.h + 2 * g.P), dim3(256), 0,
                      s.pyr.as<const uint8_t>(), s.der.as<short2>(), v, g.P));
    }
    s.der_win = g.win, s.der_L = g.L;
    return TF_OK;
}

int check_call(tf_lk *lk, int win, int max_level, Geometry *g)
{
    TF_REQUIRE(win > 2 && win <= 255, "tf_lk: win_size %d not in [3, 255]", win);
    TF_REQUIRE(max_level >= 0, "tf_lk: max_level %d < 0", max_level);
    *g = make_geometry(lk->W, lk->H, win, max_level);
    TF_REQUIRE(g->L < MAX_LEVELS, "tf_lk: %d pyramid levels (at most %d)", g->L + 1, MAX_LEVELS);
    return TF_OK;
}

} // namespace

TF_API int tf_lk_create(tf_lk **out, int width, int height, int frame_slots, int max_pairs)
{
    TF_REQUIRE(out, "tf_lk_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(width >= 1 && height >= 1 && width < 65536 && height < 65536 && (long long)width * height < (1ll << 31),
               "tf_lk_create: bad size %dx%d", width, height);
    TF_REQUIRE(frame_slots >= 2, "tf_lk_create: frame_slots %d < 2", frame_slots);
    TF_REQUIRE(max_pairs >= 1 && max_pairs <= MAX_PAIRS, "tf_lk_create: max_pairs %d not in [1, %d]", max_pairs, MAX_PAIRS);
    TF_TRY(ensure_init());
    auto lk = make_handle<tf_lk>();
    TF_REQUIRE(lk, "tf_lk_create: out of memory");
    lk->W = width, lk->H = height, lk->n_slots = frame_slots, lk->max_pairs = max_pairs;
    lk->slots.reset(new (std::nothrow) tf_lk::Slot[frame_slots]);
    TF_REQUIRE(lk->slots, "tf_lk_create: out of memory");
    const size_t npx = (size_t)width * height;
    TF_TRY(lk->frames.alloc((size_t)frame_slots * npx));
    TF_TRY(lk->flow.alloc((size_t)max_pairs * npx * sizeof(float2)));
    TF_TRY(lk->stats.alloc((size_t)max_pairs * MAX_LEVELS * 2 * sizeof(unsigned long long)));
    lk->host_stats.assign((size_t)max_pairs * MAX_LEVELS * 2, 0);
    *out = lk.release();
    return TF_OK;
}

TF_API void tf_lk_destroy(tf_lk *lk)
{
    if (lk)
        (void)hipStreamSynchronize(stream()); // kernels of the handle's last call may still read its buffers
    delete lk;
}

TF_API int tf_lk_set_frame(tf_lk *lk, int slot, const uint8_t *grey, ptrdiff_t stride)
{
    TF_REQUIRE(lk && grey, "tf_lk_set_frame: null pointer");
    TF_REQUIRE(slot >= 0 && slot < lk->n_slots, "tf_lk_set_frame: slot %d out of range (%d slots)", slot, lk->n_slots);
    TF_REQUIRE(stride >= lk->W, "tf_lk_set_frame: stride %td smaller than width %d", stride, lk->W);
    uint8_t *dst = lk->frames.as<uint8_t>() + (size_t)slot * lk->W * lk->H;
    TF_HIP(hipMemcpy2DAsync(dst, lk->W, grey, (size_t)stride, lk->W, lk->H, hipMemcpyHostToDevice, stream()));
    TF_HIP(hipStreamSynchronize(stream())); // the host frame is borrowed for this call only
    tf_lk::Slot &s = lk->slots[slot];
    s.pyr_win = s.pyr_L = s.der_win = s.der_L = -1;
    return TF_OK;
}

// cv.py:461-466 on the device, as tf_fb_set_frame_bgr: nearest-neighbour resize and BGR -> grey into the slot
TF_API int tf_lk_set_frame_bgr(tf_lk *lk, int slot, const uint8_t *bgr, int src_width, int src_height, ptrdiff_t stride)
{
    TF_REQUIRE(lk && bgr, "tf_lk_set_frame_bgr: null pointer");
    TF_REQUIRE(slot >= 0 && slot < lk->n_slots, "tf_lk_set_frame_bgr: slot %d out of range (%d slots)", slot, lk->n_slots);
    TF_REQUIRE(src_width >= 1 && src_height >= 1 && (long long)src_width * src_height < (1ll << 31),
               "tf_lk_set_frame_bgr: bad source size %dx%d", src_width, src_height);
    TF_REQUIRE(stride >= (ptrdiff_t)3 * src_width, "tf_lk_set_frame_bgr: stride %td smaller than a row of %d BGR pixels",
               stride, src_width);
    const size_t row = (size_t)3 * src_width, need = row * src_height;
    if (lk->bgr_stage.bytes < need)
        TF_TRY(lk->bgr_stage.alloc(need));
    uint8_t *dst = lk->frames.as<uint8_t>() + (size_t)slot * lk->W * lk->H;
    TF_HIP(hipMemcpy2DAsync(lk->bgr_stage.p, row, bgr, (size_t)stride, row, src_height, hipMemcpyHostToDevice, stream()));
    TF_TRY(tf_frame_grey_dev(lk->bgr_stage.p, src_width, src_height, dst, lk->W, lk->H));
    TF_HIP(hipStreamSynchronize(stream()));
    tf_lk::Slot &s = lk->slots[slot];
    s.pyr_win = s.pyr_L = s.der_win = s.der_L = -1;
    return TF_OK;
}

TF_API int tf_lk_calc_slots(tf_lk *lk, int win_size, int max_level, int step, int n_pairs, const int *prev_slots,
                            const int *next_slots, int collect_stats)
{
    TF_REQUIRE(lk && prev_slots && next_slots, "tf_lk_calc_slots: null pointer");
    TF_REQUIRE(n_pairs >= 1 && n_pairs <= lk->max_pairs, "tf_lk_calc_slots: %d pairs (handle takes 1..%d)", n_pairs,
               lk->max_pairs);
    TF_REQUIRE(step >= 1, "tf_lk_calc_slots: step %d < 1", step);
    Geometry g;
    TF_TRY(check_call(lk, win_size, max_level, &g));
    for (int i = 0; i < n_pairs; i++)
        TF_REQUIRE(prev_slots[i] >= 0 && prev_slots[i] < lk->n_slots && next_slots[i] >= 0 && next_slots[i] < lk->n_slots,
                   "tf_lk_calc_slots: pair %d: slots (%d, %d) out of range (%d slots)", i, prev_slots[i], next_slots[i],
                   lk->n_slots);
    PairPtrs pp;
    TrackOut to;
    std::memset(&pp, 0, sizeof pp);
    std::memset(&to, 0, sizeof to);
    for (int i = 0; i < n_pairs; i++) {
        TF_TRY(ensure_derivs(lk, prev_slots[i], g));
        TF_TRY(ensure_pyramid(lk, next_slots[i], g));
    }
    const size_t npx = (size_t)lk->W * lk->H;
    for (int i = 0; i < n_pairs; i++) {
        pp.I[i] = lk->slots[prev_slots[i]].pyr.as<const uint8_t>();
        pp.D[i] = lk->slots[prev_slots[i]].der.as<const short2>();
        pp.J[i] = lk->slots[next_slots[i]].pyr.as<const uint8_t>();
        to.flow[i] = lk->flow.as<float2>() + (size_t)i * npx;
    }
    if (collect_stats) {
        to.stats = lk->stats.as<unsigned long long>();
        TF_HIP(hipMemsetAsync(to.stats, 0, (size_t)n_pairs * MAX_LEVELS * 2 * sizeof(unsigned long long), stream()));
    }
    const int gw = (lk->W + step - 1) / step, gh = (lk->H + step - 1) / step;
    const int npts = gw * gh;
    TF_TRY(launch("lk_track", k_lk_track, dim3(cdiv(npts, TRACK_BX), n_pairs), dim3(TRACK_BX), 0, g, pp, to, lk->W,
                  lk->H, step, gw, npts));
    lk->last_pairs = n_pairs, lk->last_L = g.L;
    if (collect_stats) {
        TF_HIP(hipMemcpyAsync(lk->host_stats.data(), to.stats, (size_t)n_pairs * MAX_LEVELS * 2 * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, stream()));
        TF_HIP(hipStreamSynchronize(stream()));
    } else {
        std::fill(lk->host_stats.begin(), lk->host_stats.end(), 0ull);
    }
    return TF_OK;
}

TF_API int tf_lk_get_flow(tf_lk *lk, int pair, float *flow_out)
{
    TF_REQUIRE(lk && flow_out, "tf_lk_get_flow: null pointer");
    TF_REQUIRE(pair >= 0 && pair < lk->last_pairs, "tf_lk_get_flow: pair %d was not computed by the last call", pair);
    const size_t bytes = (size_t)lk->W * lk->H * sizeof(float2);
    TF_HIP(hipMemcpyAsync(flow_out, (char *)lk->flow.p + (size_t)pair * bytes, bytes, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

TF_API int tf_lk_flow_ptr(tf_lk *lk, int pair, void **dev)
{
    TF_REQUIRE(lk && dev, "tf_lk_flow_ptr: null pointer");
    TF_REQUIRE(pair >= 0 && pair < lk->last_pairs, "tf_lk_flow_ptr: pair %d was not computed by the last call", pair);
    *dev = (char *)lk->flow.p + (size_t)pair * lk->W * lk->H * sizeof(float2);
    return TF_OK;
}

TF_API int tf_lk_stats(tf_lk *lk, int pair, int *n_levels, unsigned long long *sum_max)
{
    TF_REQUIRE(lk && n_levels && sum_max, "tf_lk_stats: null pointer");
    TF_REQUIRE(pair >= 0 && pair < lk->last_pairs, "tf_lk_stats: pair %d was not computed by the last call", pair);
    *n_levels = lk->last_L + 1;
    for (int k = 0; k < MAX_LEVELS * 2; k++)
        sum_max[k] = lk->host_stats[(size_t)pair * MAX_LEVELS * 2 + k];
    return TF_OK;
}

TF_API int tf_lk_stage_pyramid(tf_lk *lk, int slot, int win_size, int max_level, int level, uint8_t *out)
{
    TF_REQUIRE(lk && out, "tf_lk_stage_pyramid: null pointer");
    TF_REQUIRE(slot >= 0 && slot < lk->n_slots, "tf_lk_stage_pyramid: slot %d out of range", slot);
    Geometry g;
    TF_TRY(check_call(lk, win_size, max_level, &g));
    TF_REQUIRE(level >= 0 && level <= g.L, "tf_lk_stage_pyramid: level %d not in [0, %d]", level, g.L);
    TF_TRY(ensure_pyramid(lk, slot, g));
    const Level &v = g.lv[level];
    const size_t n = (size_t)v.stride * (v.h + 2 * g.P);
    const uint8_t *src = lk->slots[slot].pyr.as<const uint8_t>() + (v.origin - (long long)g.P * v.stride - g.P);
    TF_HIP(hipMemcpyAsync(out, src, n, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

TF_API int tf_lk_stage_scharr(tf_lk *lk, int slot, int win_size, int max_level, int level, int16_t *out)
{
    TF_REQUIRE(lk && out, "tf_lk_stage_scharr: null pointer");
    TF_REQUIRE(slot >= 0 && slot < lk->n_slots, "tf_lk_stage_scharr: slot %d out of range", slot);
    Geometry g;
    TF_TRY(check_call(lk, win_size, max_level, &g));
    TF_REQUIRE(level >= 0 && level <= g.L, "tf_lk_stage_scharr: level %d not in [0, %d]", level, g.L);
    TF_TRY(ensure_derivs(lk, slot, g));
    const Level &v = g.lv[level];
    const size_t n = (size_t)v.stride * (v.h + 2 * g.P);
    const short2 *src = lk->slots[slot].der.as<const short2>() + (v.origin - (long long)g.P * v.stride - g.P);
    TF_HIP(hipMemcpyAsync(out, src, n * sizeof(short2), hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

TF_API int tf_lk_stage_trace(tf_lk *lk, int prev_slot, int next_slot, int win_size, int max_level, float x, float y,
                             float *out)
{
    TF_REQUIRE(lk && out, "tf_lk_stage_trace: null pointer");
    TF_REQUIRE(prev_slot >= 0 && prev_slot < lk->n_slots && next_slot >= 0 && next_slot < lk->n_slots,
               "tf_lk_stage_trace: slots (%d, %d) out of range", prev_slot, next_slot);
    Geometry g;
    TF_TRY(check_call(lk, win_size, max_level, &g));
    TF_TRY(ensure_derivs(lk, prev_slot, g));
    TF_TRY(ensure_pyramid(lk, next_slot, g));
    if (lk->bgr_stage.bytes < MAX_LEVELS * sizeof(float4))
        TF_TRY(lk->bgr_stage.alloc(MAX_LEVELS * sizeof(float4)));
    float4 *tr = lk->bgr_stage.as<float4>();
    TF_TRY(launch("lk_trace", k_lk_trace, dim3(1), dim3(64), 0, g, lk->slots[prev_slot].pyr.as<const uint8_t>(),
                  lk->slots[next_slot].pyr.as<const uint8_t>(), lk->slots[prev_slot].der.as<const short2>(), x, y, tr));
    TF_HIP(hipMemcpyAsync(out, tr, (size_t)(g.L + 1) * sizeof(float4), hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}
