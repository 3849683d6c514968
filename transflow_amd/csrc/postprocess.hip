// B1: FlowSource.post_process (source.py:337-363) on a device flow -- the clip, the FORWARD scatter (last write wins)
// and its resolve, in float32 or (after a float64 convolution kernel, :344-348) float64 -- and the flow filters / mask
// multiply that precede it (filters.py:36-72).  One implementation for every caller: the tf_fb_post_process* entry
// points (farneback.hip) and the handle-free tf_flow_post_process*_dev bring their own winner buffer.  Also the
// convolution kernel fused with what follows it (tf_flow_convolve_post_process_dev) and the rounding of a float64 flow
// for the compositor's layers (tf_flow_narrow_dev).
#include <cstring>

#include "common.h"

using namespace tf;

namespace {

// numpy.clip, to the bit: min(max(v, lo), hi) as comparisons (v > lo ? v : lo, then t < hi ? t : hi), so a -0.0 meeting
// a bound of 0 comes out as the bound's +0.0 on either side; the hardware's min / max order -0 below +0 and would keep
// the -0.0 at an upper bound of 0 (the last column / row).  Painted motion-vector flows are full of -0.0.
template <typename T> __device__ __forceinline__ T clip_np(T v, T lo, T hi)
{
    if (v != v)
        return v;
    const T t = v > lo ? v : lo;
    return t < hi ? t : hi;
}

template <typename T2> __device__ __forceinline__ T2 clip_to_frame(T2 f, int i, int j, int W, int H)
{
    typedef decltype(f.x) T;
    f.x = clip_np<T>(f.x, (T)(-j), (T)(W - 1 - j));
    f.y = clip_np<T>(f.y, (T)(-i), (T)(H - 1 - i));
    return f;
}

__device__ __forceinline__ int rint_i(float v) { return (int)rintf(v); }
__device__ __forceinline__ int rint_i(double v) { return (int)rint(v); }

template <typename T2> __global__ void k_pp_clip(T2 *flow, int W, int H, FastDiv dw)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= W * H)
        return;
    const int i = (int)fast_div((uint32_t)t, dw);
    flow[t] = clip_to_frame(flow[t], i, t - i * W, W, H);
}

// source.py:350-358: every moving source p claims target p+d; numpy.put writes in
// ascending p, so the largest p wins -> atomicMax on the source index.
template <typename T2>
__global__ void k_pp_fwd_scatter(const T2 *__restrict__ flow, int *__restrict__ winner, int W, int H, FastDiv dw)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = W * H;
    if (t >= N)
        return;
    const int i = (int)fast_div((uint32_t)t, dw);
    T2 f = clip_to_frame(flow[t], i, t - i * W, W, H);
    int ix = rint_i(f.x), iy = rint_i(f.y);
    int d = iy * W + ix;
    if (d == 0)
        return;
    int target = clampi(t + d, 0, N - 1); // mode="clip"
    atomicMax(&winner[target], t);
}

template <typename T2>
__global__ void k_pp_fwd_resolve(T2 *__restrict__ flow, const int *__restrict__ winner, int W, int H, FastDiv dw)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= W * H)
        return;
    typedef decltype(flow[0].x) T;
    int w = winner[t];
    int src = w >= 0 ? w : t;
    const int i = (int)fast_div((uint32_t)t, dw), j = t - i * W;
    const int si = (int)fast_div((uint32_t)src, dw);
    T2 f;
    f.x = (T)(src - si * W - j); // source.py:359-360
    f.y = (T)(si - i);
    flow[t] = clip_to_frame(f, i, j, W, H); // :361-362
}

// The optional pre-steps of post_process: filters.py:36-72 and the mask multiply of
// source.py:342-343, per pixel, in numpy's arithmetic (float32 for weak scalars, float64 for
// numpy.float64 values; numpy.linalg.norm of a float32 pair is sqrt(x*x + y*y) in float32).
struct FlowOps {
    int n;
    tf_flow_op op[TF_MAX_FLOW_OPS];
};

__global__ void k_pp_ops(float2 *__restrict__ flow, const float *__restrict__ mask, int N, FlowOps ops)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N)
        return;
    float2 f = flow[t];
    for (int i = 0; i < ops.n; i++) {
        const int kind = ops.op[i].kind, wide = ops.op[i].wide;
        const double v = ops.op[i].value;
        if (kind == TF_FLOW_SCALE) {
            if (wide) {
                f.x = (float)((double)f.x * v);
                f.y = (float)((double)f.y * v);
            } else {
                f.x = f.x * (float)v;
                f.y = f.y * (float)v;
            }
        } else {
            const float norm = sqrtf(f.x * f.x + f.y * f.y);
            if (kind == TF_FLOW_THRESHOLD) {
                const bool hit = wide ? ((double)norm <= v) : (norm <= (float)v);
                if (hit)
                    f = make_float2(0.f, 0.f);
            } else { // clip: factors stay 1.0 (float64) where the norm is below the threshold
                const bool hit = wide ? ((double)norm >= v) : (norm >= (float)v);
                if (hit) {
                    const double factor = wide ? v / (double)norm : (double)((float)v / norm);
                    f.x = (float)((double)f.x * factor);
                    f.y = (float)((double)f.y * factor);
                }
            }
        }
    }
    if (mask) {
        const float m = mask[t];
        f.x = m * f.x;
        f.y = m * f.y;
    }
    flow[t] = f;
}

// ---- Out of place, and leaving the chain state (tf_flow_post_process_chain_dev): the same arithmetic as the kernels
// above, on a flow that is read once from `src` (a method handle's own buffer, left as it is) and written to `dst`, and
// -- where `chain` is given -- to the buffer the next call's initial flow is read from: the reference's prev_flow, which
// sees the filters and, because the mask multiply makes a new array (source.py:342-343), not the mask.
// A lane works on PX adjacent pixels: 2 (one 16-byte access per flow) where every buffer is 16-byte aligned (a pair of
// a handle with an odd pixel count is not), else 1; a last lane of 2 that holds a single pixel takes it alone.

// k_pp_ops's filters on one pixel
__device__ __forceinline__ float2 ops_px(float2 f, const FlowOps &ops)
{
    for (int i = 0; i < ops.n; i++) {
        const int kind = ops.op[i].kind, wide = ops.op[i].wide;
        const double v = ops.op[i].value;
        if (kind == TF_FLOW_SCALE) {
            if (wide) {
                f.x = (float)((double)f.x * v);
                f.y = (float)((double)f.y * v);
            } else {
                f.x = f.x * (float)v;
                f.y = f.y * (float)v;
            }
        } else {
            const float norm = sqrtf(f.x * f.x + f.y * f.y);
            if (kind == TF_FLOW_THRESHOLD) {
                const bool hit = wide ? ((double)norm <= v) : (norm <= (float)v);
                if (hit)
                    f = make_float2(0.f, 0.f);
            } else {
                const bool hit = wide ? ((double)norm >= v) : (norm >= (float)v);
                if (hit) {
                    const double factor = wide ? v / (double)norm : (double)((float)v / norm);
                    f.x = (float)((double)f.x * factor);
                    f.y = (float)((double)f.y * factor);
                }
            }
        }
    }
    return f;
}

template <int PX> struct PxLane {
    unsigned t0; // the lane's first pixel
    int n;       // how many it holds: PX, or 1 at an odd end
    __device__ __forceinline__ PxLane(unsigned N) : t0((blockIdx.x * 256u + threadIdx.x) * PX), n(t0 >= N ? 0 : (N - t0 >= PX ? PX : 1)) {}
    template <typename T> __device__ __forceinline__ void load(const T *__restrict__ p, T (&v)[PX]) const
    {
        if (PX == 2 && n == 2) {
            struct alignas(2 * sizeof(T)) Two {
                T a, b;
            };
            const Two two = *(const Two *)(p + t0);
            v[0] = two.a, v[PX - 1] = two.b;
        } else {
            v[0] = v[PX - 1] = p[t0]; // (the second of an odd end: worked on, never stored)
        }
    }
    template <typename T> __device__ __forceinline__ void store(T *__restrict__ p, const T (&v)[PX]) const
    {
        if (PX == 2 && n == 2) {
            struct alignas(2 * sizeof(T)) Two {
                T a, b;
            };
            *(Two *)(p + t0) = Two{v[0], v[PX - 1]};
        } else {
            p[t0] = v[0];
        }
    }
};

// the filters, the mask and the chain value of the lane's pixels: f comes back as what the direction handling reads
template <int PX>
__device__ __forceinline__ void chain_head(const PxLane<PX> &ln, float2 (&f)[PX], float2 *__restrict__ chain,
                                           const float *__restrict__ mask, const FlowOps &ops)
{
#pragma unroll
    for (int k = 0; k < PX; k++)
        f[k] = ops_px(f[k], ops);
    if (!mask)
        return;
    if (chain)
        ln.store(chain, f);
    float m[PX];
    ln.load(mask, m);
#pragma unroll
    for (int k = 0; k < PX; k++) {
        f[k].x = m[k] * f[k].x;
        f[k].y = m[k] * f[k].y;
    }
}

// BACKWARD (CLIP) and no direction handling: one pass
template <int PX, bool CLIP>
__global__ void __launch_bounds__(256)
    k_pp_chain_line(const float2 *__restrict__ src, float2 *__restrict__ dst, float2 *__restrict__ chain,
                    const float *__restrict__ mask, int W, int H, FastDiv dw, FlowOps ops)
{
    const PxLane<PX> ln((unsigned)(W * H));
    if (ln.n == 0)
        return;
    float2 f[PX];
    ln.load(src, f);
    chain_head(ln, f, chain, mask, ops);
    if (CLIP) {
#pragma unroll
        for (int k = 0; k < PX; k++) {
            const int i = (int)fast_div(ln.t0 + k, dw);
            f[k] = clip_to_frame(f[k], i, (int)(ln.t0 + k) - i * W, W, H);
        }
    }
    ln.store(dst, f);
    if (chain && !mask)
        ln.store(chain, f);
}

// FORWARD, first pass: k_pp_fwd_scatter on the filtered and masked value, which stays in registers
template <int PX>
__global__ void __launch_bounds__(256)
    k_pp_chain_scatter(const float2 *__restrict__ src, float2 *__restrict__ chain, const float *__restrict__ mask,
                       int *__restrict__ winner, int W, int H, FastDiv dw, FlowOps ops)
{
    const int N = W * H;
    const PxLane<PX> ln((unsigned)N);
    if (ln.n == 0)
        return;
    float2 f[PX];
    ln.load(src, f);
    chain_head(ln, f, chain, mask, ops);
#pragma unroll
    for (int k = 0; k < PX; k++) {
        if (k >= ln.n)
            break;
        const int t = (int)ln.t0 + k, i = (int)fast_div((uint32_t)t, dw);
        const float2 c = clip_to_frame(f[k], i, t - i * W, W, H);
        const int d = rint_i(c.y) * W + rint_i(c.x);
        if (d != 0)
            atomicMax(&winner[clampi(t + d, 0, N - 1)], t);
    }
}

// FORWARD, second pass: k_pp_fwd_resolve into dst, and into the chain where no mask set it in the first pass
template <int PX>
__global__ void __launch_bounds__(256)
    k_pp_chain_resolve(float2 *__restrict__ dst, float2 *__restrict__ chain, const int *__restrict__ winner, int W, int H,
                       FastDiv dw)
{
    const PxLane<PX> ln((unsigned)(W * H));
    if (ln.n == 0)
        return;
    int w[PX];
    ln.load(winner, w);
    float2 f[PX];
#pragma unroll
    for (int k = 0; k < PX; k++) {
        const int t = (int)ln.t0 + k; // (past the end at an odd end: computed, never stored)
        const int src = w[k] >= 0 ? w[k] : t;
        const int i = (int)fast_div((uint32_t)t, dw), j = t - i * W;
        const int si = (int)fast_div((uint32_t)src, dw);
        f[k] = clip_to_frame(make_float2((float)(src - si * W - j), (float)(si - i)), i, j, W, H);
    }
    ln.store(dst, f);
    if (chain)
        ln.store(chain, f);
}

template <int PX>
int chain_launch(const float2 *src, float2 *dst, float2 *chain, int W, int H, int direction, const FlowOps &fo,
                 const float *mask, int *winner)
{
    const size_t N = (size_t)W * H;
    const dim3 grid(cdiv(N, 256 * PX)), block(256);
    const FastDiv dw = fast_div_setup((uint32_t)W);
    if (direction == 0) {
        TF_HIP(hipMemsetAsync(winner, 0xFF, N * 4, stream()));
        TF_TRY(launch("flow_pp_chain_scatter", k_pp_chain_scatter<PX>, grid, block, 0, src, mask ? chain : nullptr, mask,
                      winner, W, H, dw, fo));
        return launch("flow_pp_chain_resolve", k_pp_chain_resolve<PX>, grid, block, 0, dst, mask ? nullptr : chain,
                      (const int *)winner, W, H, dw);
    }
    if (direction == 1)
        return launch("flow_pp_chain_line", k_pp_chain_line<PX, true>, grid, block, 0, src, dst, chain, mask, W, H, dw, fo);
    return launch("flow_pp_chain_line", k_pp_chain_line<PX, false>, grid, block, 0, src, dst, chain, mask, W, H, dw, fo);
}

// ---- The convolution tail (tf_flow_convolve_post_process_dev): source.py:344-362 out of place and in one pass over
// the flow.  The sums are k_flow_convolve's / k_flow_convolve_tiled's (flowops.hip), statement for statement -- kernel
// rows j, then columns k, every product and sum rounded in T, the fill value taking part -- so the convolved vector is
// theirs to the bit; what follows it in T happens in registers.  END says what: the plain store (no direction), the
// clip and the store (BACKWARD: k_pp_clip's statement), or the clip, the round and the claim in the winner map (FORWARD:
// k_pp_fwd_scatter's statements; the convolved flow is never stored, k_pp_tail_resolve writes the output).
template <typename T> struct Vec2;
template <> struct Vec2<float> {
    typedef float2 type;
};
template <> struct Vec2<double> {
    typedef double2 type;
};

enum TailEnd { TAIL_STORE, TAIL_CLIP, TAIL_SCATTER };

constexpr int CT_TW = 64, CT_TH = 16; // k_flow_convolve_tiled's tile: 64 x 16 outputs per block of 256

template <typename T, int END>
__device__ __forceinline__ void tail_end(T sx, T sy, int i, int j, int W, int H, typename Vec2<T>::type *__restrict__ out,
                                         int *__restrict__ winner)
{
    typename Vec2<T>::type r;
    r.x = sx;
    r.y = sy;
    const int t = i * W + j;
    if (END != TAIL_STORE)
        r = clip_to_frame(r, i, j, W, H);
    if (END != TAIL_SCATTER) {
        out[t] = r;
        return;
    }
    const int d = rint_i(r.y) * W + rint_i(r.x);
    if (d != 0)
        atomicMax(&winner[clampi(t + d, 0, W * H - 1)], t); // mode="clip"; the largest source wins
}

template <typename T, int END>
__global__ void __launch_bounds__(256)
    k_conv_tail(const float2 *__restrict__ flow, const T *__restrict__ kern, int kh, int kw,
                typename Vec2<T>::type *__restrict__ out, int *__restrict__ winner, int W, int H)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)W * H)
        return;
    const int n = (int)(t % W), m = (int)(t / W);
    const int oy = (kh - 1) >> 1, ox = (kw - 1) >> 1;
    T sx = 0, sy = 0;
    for (int j = 0; j < kh; j++) {
        const int y = m + oy - j;
        const bool row_in = y >= 0 && y < H;
        for (int k = 0; k < kw; k++) {
            const int x = n + ox - k;
            const T hv = kern[j * kw + k];
            T vx = 0, vy = 0;
            if (row_in && x >= 0 && x < W) {
                const float2 f = flow[(size_t)y * W + x];
                vx = (T)f.x;
                vy = (T)f.y;
            }
            sx = sx + hv * vx; // the fill value takes part: 0 * h
            sy = sy + hv * vy;
        }
    }
    tail_end<T, END>(sx, sy, m, n, W, H, out, winner);
}

template <typename T, int END>
__global__ void __launch_bounds__(256)
    k_conv_tail_tiled(const float2 *__restrict__ flow, const T *__restrict__ kern, int kh, int kw,
                      typename Vec2<T>::type *__restrict__ out, int *__restrict__ winner, int W, int H)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_ct[];
    const int LW = CT_TW + kw - 1, LH = CT_TH + kh - 1;
    float2 *tile = reinterpret_cast<float2 *>(s_ct);
    T *sk = reinterpret_cast<T *>(s_ct + (((size_t)LW * LH * sizeof(float2) + 15) & ~(size_t)15));
    const int x0 = blockIdx.x * CT_TW, y0 = blockIdx.y * CT_TH;
    const int oy = (kh - 1) >> 1, ox = (kw - 1) >> 1;
    // tile (ry, rx) <-> image (y0 + oy - (kh-1) + ry, x0 + ox - (kw-1) + rx)
    const int ty0 = y0 + oy - (kh - 1), tx0 = x0 + ox - (kw - 1);
    for (int idx = threadIdx.x; idx < LW * LH; idx += 256) {
        const int ry = idx / LW, rx = idx - ry * LW;
        const int y = ty0 + ry, x = tx0 + rx;
        tile[idx] = (y >= 0 && y < H && x >= 0 && x < W) ? flow[(size_t)y * W + x] : make_float2(0.f, 0.f);
    }
    for (int idx = threadIdx.x; idx < kh * kw; idx += 256)
        sk[idx] = kern[idx];
    __syncthreads();
    const int tx = threadIdx.x & 63, tq = threadIdx.x >> 6;
    T sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0};
    for (int j = 0; j < kh; j++) {
        for (int k = 0; k < kw; k++) {
            const T hv = sk[j * kw + k];
            const float2 *p = tile + (tq + (kh - 1) - j) * LW + tx + (kw - 1) - k;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float2 f = p[4 * q * LW];
                sx[q] = sx[q] + hv * (T)f.x;
                sy[q] = sy[q] + hv * (T)f.y;
            }
        }
    }
    const int x = x0 + tx;
    if (x >= W)
        return;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int y = y0 + tq + 4 * q;
        if (y < H)
            tail_end<T, END>(sx[q], sy[q], y, x, W, H, out, winner);
    }
}

// FORWARD's second launch: k_pp_fwd_resolve's statements, written to the output instead of over the flow
template <typename T2>
__global__ void __launch_bounds__(256) k_pp_tail_resolve(T2 *__restrict__ dst, const int *__restrict__ winner, int W, int H, FastDiv dw)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= W * H)
        return;
    typedef decltype(dst[0].x) T;
    const int w = winner[t];
    const int src = w >= 0 ? w : t;
    const int i = (int)fast_div((uint32_t)t, dw), j = t - i * W;
    const int si = (int)fast_div((uint32_t)src, dw);
    T2 f;
    f.x = (T)(src - si * W - j); // source.py:359-360
    f.y = (T)(si - i);
    dst[t] = clip_to_frame(f, i, j, W, H); // :361-362
}

template <typename T, int END>
int conv_tail_launch(const float2 *src, const T *kern, int kh, int kw, typename Vec2<T>::type *dst, int *winner, int W, int H)
{
    const size_t N = (size_t)W * H;
    // tf_flow_convolve_dev's rule: the tiled form where the float2 tile (padded to 16 bytes) and the kernel fit 64 KB
    const size_t tile_bytes = (((size_t)(CT_TW + kw - 1) * (CT_TH + kh - 1) * sizeof(float2) + 15) & ~(size_t)15) +
                              (size_t)kh * kw * sizeof(T);
    const char *name = sizeof(T) == 8 ? "flow_conv_tail_f64" : "flow_conv_tail_f32";
    static const bool no_tiles = tune("TF_CONV_NO_TILES", 0) != 0;
    if (tile_bytes <= 64 * 1024 && !no_tiles)
        return launch(name, k_conv_tail_tiled<T, END>, dim3(cdiv(W, CT_TW), cdiv(H, CT_TH)), dim3(256), tile_bytes, src, kern,
                      kh, kw, dst, winner, W, H);
    return launch(name, k_conv_tail<T, END>, dim3(cdiv(N, 256)), dim3(256), 0, src, kern, kh, kw, dst, winner, W, H);
}

template <typename T>
int conv_tail(const float2 *src, const T *kern, int kh, int kw, typename Vec2<T>::type *dst, int W, int H, int direction,
              int *winner)
{
    if (direction < 0)
        return conv_tail_launch<T, TAIL_STORE>(src, kern, kh, kw, dst, nullptr, W, H);
    if (direction == 1)
        return conv_tail_launch<T, TAIL_CLIP>(src, kern, kh, kw, dst, nullptr, W, H);
    const size_t N = (size_t)W * H;
    TF_HIP(hipMemsetAsync(winner, 0xFF, N * 4, stream()));
    TF_TRY((conv_tail_launch<T, TAIL_SCATTER>(src, kern, kh, kw, dst, winner, W, H)));
    return launch("flow_conv_tail_resolve", k_pp_tail_resolve<typename Vec2<T>::type>, dim3(cdiv(N, 256)), dim3(256), 0, dst,
                  (const int *)winner, W, H, fast_div_setup((uint32_t)W));
}

// float32(rint(x)) or float32(floor(x)) of a float64 flow, in double (numpy.round / numpy.floor of the float64 array, then
// the cast: movement.py:21, sum.py:10): ties to even, -0.5 -> -0.0, NaN stays NaN.  VEC: a lane takes two pixels -- four
// values, 32 bytes in and 16 out -- where both buffers are 16-byte aligned; what is left of the end goes value by value.
template <int FLOOR> __device__ __forceinline__ float narrow1(double v) { return (float)(FLOOR ? floor(v) : rint(v)); }

template <int FLOOR, bool VEC>
__global__ void __launch_bounds__(256) k_flow_narrow(const double *__restrict__ src, float *__restrict__ dst, size_t n)
{
    const size_t lane = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (!VEC) {
        if (lane < n)
            dst[lane] = narrow1<FLOOR>(src[lane]);
        return;
    }
    const size_t v0 = lane * 4;
    if (v0 >= n)
        return;
    if (v0 + 4 <= n) {
        const double2 a = *reinterpret_cast<const double2 *>(src + v0), b = *reinterpret_cast<const double2 *>(src + v0 + 2);
        *reinterpret_cast<float4 *>(dst + v0) =
            make_float4(narrow1<FLOOR>(a.x), narrow1<FLOOR>(a.y), narrow1<FLOOR>(b.x), narrow1<FLOOR>(b.y));
        return;
    }
    for (size_t v = v0; v < n; v++)
        dst[v] = narrow1<FLOOR>(src[v]);
}

template <typename T2> int scatter(const T2 *flow, int W, int H, int *winner, const PpLabels &lb)
{
    const size_t N = (size_t)W * H;
    if (N == 0)
        return TF_OK;
    TF_REQUIRE(winner, "post_process: FORWARD needs a winner buffer of 4 bytes per pixel");
    TF_HIP(hipMemsetAsync(winner, 0xFF, N * 4, stream()));
    return launch(lb.fwd_scatter, k_pp_fwd_scatter<T2>, dim3(cdiv(N, 256)), dim3(256), 0, flow, winner, W, H,
                  fast_div_setup((uint32_t)W));
}

template <typename T2> int direction_t(T2 *flow, int W, int H, int direction, int *winner, const PpLabels &lb)
{
    const size_t N = (size_t)W * H;
    if (N == 0)
        return TF_OK;
    dim3 grid(cdiv(N, 256)), block(256);
    const FastDiv dw = fast_div_setup((uint32_t)W);
    if (direction == 0) {
        TF_TRY(scatter((const T2 *)flow, W, H, winner, lb));
        return launch(lb.fwd_resolve, k_pp_fwd_resolve<T2>, grid, block, 0, flow, (const int *)winner, W, H, dw);
    }
    return launch(lb.clip, k_pp_clip<T2>, grid, block, 0, flow, W, H, dw);
}

} // namespace

namespace tf {

int pp_scatter(const float2 *flow, int W, int H, int *winner, const PpLabels &lb) { return scatter(flow, W, H, winner, lb); }

int pp_direction(void *flow, bool wide, int W, int H, int direction, int *winner, const PpLabels &lb)
{
    TF_REQUIRE(direction == 0 || direction == 1, "post_process: direction must be 0 (FORWARD) or 1 (BACKWARD), got %d",
               direction);
    if (wide)
        return direction_t((double2 *)flow, W, H, direction, winner, lb);
    return direction_t((float2 *)flow, W, H, direction, winner, lb);
}

int pp_ops(float2 *flow, int W, int H, int n_ops, const tf_flow_op *ops, const float *mask_dev, const PpLabels &lb)
{
    TF_REQUIRE(n_ops >= 0 && n_ops <= TF_MAX_FLOW_OPS, "post_process: at most %d flow filters, got %d", TF_MAX_FLOW_OPS,
               n_ops);
    TF_REQUIRE(n_ops == 0 || ops, "post_process: null filter list");
    if (n_ops == 0 && !mask_dev)
        return TF_OK;
    FlowOps fo;
    memset(&fo, 0, sizeof(fo));
    fo.n = n_ops;
    for (int i = 0; i < n_ops; i++) {
        TF_REQUIRE(ops[i].kind >= TF_FLOW_SCALE && ops[i].kind <= TF_FLOW_CLIP, "post_process: unknown filter kind %d",
                   ops[i].kind);
        fo.op[i] = ops[i];
    }
    const int N = W * H;
    return launch(lb.ops, k_pp_ops, dim3(cdiv((size_t)N, 256)), dim3(256), 0, flow, mask_dev, N, fo);
}

} // namespace tf

TF_API int tf_flow_post_process_ex_dev(void *flow_dev, int wide, int width, int height, int direction, int n_ops,
                                       const tf_flow_op *ops, const void *mask_dev, void *winner_dev)
{
    TF_REQUIRE(direction >= -1 && direction <= 1,
               "tf_flow_post_process: direction must be 0 (FORWARD), 1 (BACKWARD) or -1 (none)");
    TF_REQUIRE(width >= 0 && height >= 0 && (long long)width * height < (1ll << 31), "tf_flow_post_process: bad size");
    TF_REQUIRE(flow_dev || (size_t)width * height == 0, "tf_flow_post_process: null pointer");
    TF_REQUIRE(!wide || (n_ops == 0 && !mask_dev),
               "tf_flow_post_process: the flow filters and the mask work on float32 flows, not on a float64 one");
    TF_TRY(ensure_init());
    TF_TRY(pp_ops((float2 *)flow_dev, width, height, n_ops, ops, (const float *)mask_dev, PP_FLOW));
    if (direction < 0)
        return TF_OK;
    return pp_direction(flow_dev, wide != 0, width, height, direction, (int *)winner_dev, PP_FLOW);
}

TF_API int tf_flow_post_process_chain_dev(const void *src_dev, void *dst_dev, void *chain_dev, int width, int height,
                                          int direction, int n_ops, const tf_flow_op *ops, const void *mask_dev,
                                          void *winner_dev)
{
    TF_REQUIRE(direction >= -1 && direction <= 1,
               "tf_flow_post_process_chain: direction must be 0 (FORWARD), 1 (BACKWARD) or -1 (none)");
    TF_REQUIRE(width >= 0 && height >= 0 && (long long)width * height < (1ll << 31), "tf_flow_post_process_chain: bad size");
    TF_REQUIRE(n_ops >= 0 && n_ops <= TF_MAX_FLOW_OPS, "tf_flow_post_process_chain: at most %d flow filters, got %d",
               TF_MAX_FLOW_OPS, n_ops);
    TF_REQUIRE(n_ops == 0 || ops, "tf_flow_post_process_chain: null filter list");
    if ((size_t)width * height == 0)
        return TF_OK;
    TF_REQUIRE(src_dev && dst_dev, "tf_flow_post_process_chain: null pointer");
    TF_REQUIRE(src_dev != dst_dev && src_dev != chain_dev && dst_dev != chain_dev,
               "tf_flow_post_process_chain: src, dst and chain must be three buffers");
    TF_REQUIRE(direction != 0 || winner_dev, "tf_flow_post_process_chain: FORWARD needs a winner buffer of 4 bytes per pixel");
    FlowOps fo;
    memset(&fo, 0, sizeof(fo));
    fo.n = n_ops;
    for (int i = 0; i < n_ops; i++) {
        TF_REQUIRE(ops[i].kind >= TF_FLOW_SCALE && ops[i].kind <= TF_FLOW_CLIP, "tf_flow_post_process_chain: unknown filter kind %d",
                   ops[i].kind);
        fo.op[i] = ops[i];
    }
    TF_TRY(ensure_init());
    const uintptr_t flows = (uintptr_t)src_dev | (uintptr_t)dst_dev | (uintptr_t)chain_dev;
    const uintptr_t words = (uintptr_t)mask_dev | (uintptr_t)winner_dev;
    TF_REQUIRE(flows % 8 == 0 && words % 4 == 0, "tf_flow_post_process_chain: misaligned buffer");
    if (flows % 16 == 0 && words % 8 == 0)
        return chain_launch<2>((const float2 *)src_dev, (float2 *)dst_dev, (float2 *)chain_dev, width, height, direction, fo,
                               (const float *)mask_dev, (int *)winner_dev);
    return chain_launch<1>((const float2 *)src_dev, (float2 *)dst_dev, (float2 *)chain_dev, width, height, direction, fo,
                           (const float *)mask_dev, (int *)winner_dev);
}

TF_API int tf_flow_post_process_dev(void *flow_dev, int wide, int width, int height, int direction, void *scratch_dev)
{
    TF_REQUIRE(direction == 0 || direction == 1, "tf_flow_post_process: direction must be 0 (FORWARD) or 1 (BACKWARD)");
    return tf_flow_post_process_ex_dev(flow_dev, wide, width, height, direction, 0, nullptr, nullptr, scratch_dev);
}

TF_API int tf_flow_convolve_post_process_dev(const void *src_dev, const void *kernel_dev, int kh, int kw, int wide,
                                             void *dst_dev, int width, int height, int direction, void *winner_dev)
{
    TF_REQUIRE(direction >= -1 && direction <= 1,
               "tf_flow_convolve_post_process: direction must be 0 (FORWARD), 1 (BACKWARD) or -1 (none)");
    TF_REQUIRE(width >= 0 && height >= 0 && (long long)width * height < (1ll << 31), "tf_flow_convolve_post_process: bad size");
    TF_REQUIRE(kh >= 1 && kw >= 1, "tf_flow_convolve_post_process: an empty convolution kernel (%d x %d)", kh, kw);
    if ((size_t)width * height == 0)
        return TF_OK;
    TF_REQUIRE(src_dev && dst_dev && kernel_dev, "tf_flow_convolve_post_process: null pointer");
    TF_REQUIRE(src_dev != dst_dev && kernel_dev != dst_dev && winner_dev != dst_dev && winner_dev != src_dev,
               "tf_flow_convolve_post_process: src, the kernel, dst and the winner map must be separate buffers");
    TF_REQUIRE(direction != 0 || winner_dev, "tf_flow_convolve_post_process: FORWARD needs a winner buffer of 4 bytes per pixel");
    TF_REQUIRE((uintptr_t)src_dev % 8 == 0 && (uintptr_t)dst_dev % (wide ? 16 : 8) == 0 &&
                   (uintptr_t)kernel_dev % (wide ? 8 : 4) == 0 && (uintptr_t)winner_dev % 4 == 0,
               "tf_flow_convolve_post_process: misaligned buffer");
    TF_TRY(ensure_init());
    if (wide)
        return conv_tail<double>((const float2 *)src_dev, (const double *)kernel_dev, kh, kw, (double2 *)dst_dev, width, height,
                                 direction, (int *)winner_dev);
    return conv_tail<float>((const float2 *)src_dev, (const float *)kernel_dev, kh, kw, (float2 *)dst_dev, width, height,
                            direction, (int *)winner_dev);
}

TF_API int tf_flow_narrow_dev(const void *src_f64_dev, void *dst_f32_dev, size_t n_values, int mode)
{
    TF_REQUIRE(mode == 0 || mode == 1, "tf_flow_narrow: mode must be 0 (rint) or 1 (floor), got %d", mode);
    if (n_values == 0)
        return TF_OK;
    TF_REQUIRE(src_f64_dev && dst_f32_dev && src_f64_dev != dst_f32_dev, "tf_flow_narrow: null or aliased pointer");
    TF_REQUIRE((uintptr_t)src_f64_dev % 8 == 0 && (uintptr_t)dst_f32_dev % 4 == 0, "tf_flow_narrow: misaligned buffer");
    TF_TRY(ensure_init());
    const double *src = (const double *)src_f64_dev;
    float *dst = (float *)dst_f32_dev;
    if (((uintptr_t)src_f64_dev | (uintptr_t)dst_f32_dev) % 16 == 0) {
        const dim3 grid(cdiv((n_values + 3) / 4, 256));
        return mode ? launch("flow_narrow", k_flow_narrow<1, true>, grid, dim3(256), 0, src, dst, n_values)
                    : launch("flow_narrow", k_flow_narrow<0, true>, grid, dim3(256), 0, src, dst, n_values);
    }
    const dim3 grid(cdiv(n_values, 256));
    return mode ? launch("flow_narrow", k_flow_narrow<1, false>, grid, dim3(256), 0, src, dst, n_values)
                : launch("flow_narrow", k_flow_narrow<0, false>, grid, dim3(256), 0, src, dst, n_values);
}
