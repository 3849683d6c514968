// LiteFlowNet: calc_optical_flow_liteflownet (transflow/flow/methods/liteflownet.py) on the GPU, float32 throughout
// by default, for all pairs of a call at once (every kernel's M or grid runs over the pairs).  A handle's precision
// (tf_lfn_set_precision) may hand the convolutions, and nothing else, to the bf16 MFMA kernel of lfn_conv_bf16.hip.
//
//   k_lfn_ingest     a decoded BGR frame of any size -> INTER_NEAREST to W x H -> the frame slot (uint8 BGR)
//   k_lfn_prep       slot -> x 1/255 -> bilinear (align_corners=False) to Hp x Wp -> minus the role's mean (NHWC)
//   k_lfn_bilinear   the image pyramid's chained resizes, and the output's x20 -> resize to W x H -> x W/Wp, H/Hp
//   k_lfn_conv<NT>   every convolution: implicit GEMM on v_mfma_f32_32x32x2_f32, M = output pixels of all images,
//                    N = Cout, K = kh kw Cin; bias, LeakyReLU and the flow heads' residual in the epilogue; reads and
//                    writes channel slices of NHWC buffers, so the concats are filled in place by their producers
//   k_lfn_deconv     the depthwise 4x4 stride-2 transposed convs (netUpflow, netUpcorr)
//   k_lfn_corr       the 7x7 correlation in the CuPy kernel's order (explicit fmaf), fused with its LeakyReLU
//   k_lfn_backwarp   grid_sample(bilinear, zeros, align_corners=True) at linspace(-1, 1) + flow * 2 / (size - 1)
//   k_lfn_mean       the flow's per-pair mean, a fixed-order reduction (one block per pair and channel)
//   k_lfn_diff       |one - backwarp(two)| over the 3 image channels and flow - mean: the first 3 channels of the
//                    Regularization concat
//   k_lfn_tail       -d^2 -> max -> exp -> sum -> netScaleX/Y of the weights times the k x k neighbourhood of the
//                    flow -> x divisor, per pixel (the unfolded flow is never stored)
//   k_lfn_copy       features into a concat slice where the concat takes them unchanged (levels 3-6)
//
// No kernel uses float atomics or split K: every output is summed by one lane in a fixed order, so flows are
// bit-identical from run to run and a pair computed in a batch equals the pair computed alone.
#include "lfn_common.h"

#include <cmath>
#include <cstring>
#include <memory>

namespace tf {
namespace lfn {

typedef float floatx16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : v * 0.1f; }

// ---- ingest and resizes ------------------------------------------------------------------------------------------

// cv2.resize(INTER_NEAREST) with dsize only: source index min(floor(dst * (1 / (dsize / src))), src - 1)
__global__ void k_lfn_ingest(const uint8_t *__restrict__ src, int Ws, int Hs, uint8_t *__restrict__ dst, int W, int H,
                             double ifx, double ify)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)W * H)
        return;
    const int x = (int)(t % W), y = (int)(t / W);
    const int sx = min((int)floor(x * ifx), Ws - 1), sy = min((int)floor(y * ify), Hs - 1);
    const uint8_t *p = src + ((size_t)sy * Ws + sx) * 3;
    dst[3 * t] = p[0], dst[3 * t + 1] = p[1], dst[3 * t + 2] = p[2];
}

// torch's bilinear source index (align_corners=False, no antialias): real = scale (dst + 0.5) - 0.5, clamped at 0;
// i0 = min(floor(real), n - 1), lambda = clamp(real - i0, 0, 1), i1 = i0 + (i0 < n - 1)
struct Tap {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ Tap bilinear_tap(int d, float scale, int n)
{
    float real = scale * ((float)d + 0.5f) - 0.5f;
    real = real < 0.f ? 0.f : real;
    Tap t;
    t.i0 = min((int)floorf(real), n - 1);
    const float lam = fminf(fmaxf(real - (float)t.i0, 0.f), 1.f);
    t.i1 = t.i0 + (t.i0 < n - 1 ? 1 : 0);
    t.w0 = 1.f - lam, t.w1 = lam;
    return t;
}

// one image of the batch per blockIdx.y: slot (uint8 BGR [H][W]) -> [Hp][Wp][3]
struct PrepArgs {
    const uint8_t *src[2 * MAX_PAIRS];
    int role[2 * MAX_PAIRS];
};
__global__ void k_lfn_prep(PrepArgs pa, int W, int H, float *__restrict__ out, int Wp, int Hp, float sx, float sy)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Wp * Hp)
        return;
    const int img = blockIdx.y;
    const int x = t % Wp, y = t / Wp;
    const Tap tx = bilinear_tap(x, sx, W), ty = bilinear_tap(y, sy, H);
    const uint8_t *s = pa.src[img];
    const float k = 1.0f / 255.0f;
    float *o = out + ((size_t)img * Hp * Wp + t) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float v00 = (float)s[((size_t)ty.i0 * W + tx.i0) * 3 + c] * k, v01 = (float)s[((size_t)ty.i0 * W + tx.i1) * 3 + c] * k;
        const float v10 = (float)s[((size_t)ty.i1 * W + tx.i0) * 3 + c] * k, v11 = (float)s[((size_t)ty.i1 * W + tx.i1) * 3 + c] * k;
        const float r0 = v00 * tx.w0 + v01 * tx.w1, r1 = v10 * tx.w0 + v11 * tx.w1;
        o[c] = (r0 * ty.w0 + r1 * ty.w1) - MEAN[pa.role[img]][c];
    }
}

// NHWC [n][h][w][C] -> [n][ho][wo][C]: in * pre, bilinear, then channel 0 x mul0 and channel 1 x mul1 (C <= 3)
__global__ void k_lfn_bilinear(const float *__restrict__ in, int C, int h, int w, float *__restrict__ out, int ho, int wo,
                               float sx, float sy, float pre, float mul0, float mul1, int apply_mul)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ho * wo)
        return;
    const int img = blockIdx.y;
    const int x = t % wo, y = t / wo;
    const Tap tx = bilinear_tap(x, sx, w), ty = bilinear_tap(y, sy, h);
    const float *s = in + (size_t)img * h * w * C;
    float *o = out + ((size_t)img * ho * wo + t) * C;
    for (int c = 0; c < C; c++) {
        const float v00 = s[((size_t)ty.i0 * w + tx.i0) * C + c] * pre, v01 = s[((size_t)ty.i0 * w + tx.i1) * C + c] * pre;
        const float v10 = s[((size_t)ty.i1 * w + tx.i0) * C + c] * pre, v11 = s[((size_t)ty.i1 * w + tx.i1) * C + c] * pre;
        const float r0 = v00 * tx.w0 + v01 * tx.w1, r1 = v10 * tx.w0 + v11 * tx.w1;
        float v = r0 * ty.w0 + r1 * ty.w1;
        if (apply_mul)
            v = v * (c == 0 ? mul0 : mul1);
        o[c] = v;
    }
}

// ---- convolution: implicit GEMM on f32 MFMA (ConvArgs: lfn_common.h; the bf16 modes: lfn_conv_bf16.hip) -------------

constexpr int CONV_BM = 128, CONV_BK = 16, CONV_THREADS = 256;

// Block: 128 output pixels x 32 NT channels, 4 waves of 32 pixels each; per K chunk of 16 the block stages A (the
// im2col rows, gathered on the fly with zero padding) and B (packed weights) in LDS and each wave runs 8 k-steps of
// NT 32x32x2 MFMAs.  Thread t gathers K column t % 16 for pixels t / 16 + 16 p (p = 0..7): 16 neighbouring lanes read
// 16 neighbouring channels.  Each output is one accumulator chain over K in ascending order.
template <int NT>
__global__ __launch_bounds__(CONV_THREADS) void k_lfn_conv(ConvArgs a)
{
    constexpr int BN = 32 * NT;
    __shared__ float As[CONV_BK][CONV_BM + 4];
    __shared__ float Bs[CONV_BK][BN + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * CONV_BM, n0 = blockIdx.y * BN;
    const int kc = tid & 15;
    const float *base[8];
    int iy0[8], ix0[8];
    const int hw = a.ho * a.wo;
#pragma unroll
    for (int p = 0; p < 8; p++) {
        const int m = m0 + (tid >> 4) + 16 * p;
        base[p] = nullptr;
        iy0[p] = ix0[p] = 0;
        if (m < a.M) {
            const int b = m / hw, r = m - b * hw, oy = r / a.wo, ox = r - oy * a.wo;
            base[p] = a.in + (size_t)b * a.hin * a.win * a.in_cs + a.in_off;
            iy0[p] = oy * a.stride - a.ph, ix0[p] = ox * a.stride - a.pw;
        }
    }
    floatx16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
        for (int r = 0; r < 16; r++)
            acc[t][r] = 0.f;
    for (int k0 = 0; k0 < a.K; k0 += CONV_BK) {
        const int k = k0 + kc;
        const bool kval = k < a.K;
        const int tap = kval ? k / a.cin : 0, ci = kval ? k - tap * a.cin : 0;
        const int ky = tap / a.kw, kx = tap - ky * a.kw;
#pragma unroll
        for (int p = 0; p < 8; p++) {
            const int iy = iy0[p] + ky, ix = ix0[p] + kx;
            float v = 0.f;
            if (kval && base[p] && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win)
                v = base[p][((size_t)iy * a.win + ix) * a.in_cs + ci];
            As[kc][(tid >> 4) + 16 * p] = v;
        }
        for (int e = tid; e < CONV_BK * BN; e += CONV_THREADS) {
            const int kk = e / BN, nn = e - kk * BN;
            Bs[kk][nn] = k0 + kk < a.K ? a.wt[(size_t)(k0 + kk) * a.npad + n0 + nn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < CONV_BK; kk += 2) {
            const float av = As[kk + (lane >> 5)][wave * 32 + (lane & 31)];
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const float bv = Bs[kk + (lane >> 5)][t * 32 + (lane & 31)];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int n = n0 + t * 32 + (lane & 31);
        if (n >= a.cout)
            continue;
        const float b = a.bias[n];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m >= a.M)
                continue;
            float v = acc[t][r] + b;
            if (a.leaky)
                v = lrelu(v);
            if (a.res)
                v = a.res[(size_t)m * a.res_cs + a.res_off + n] + v;
            a.out[(size_t)m * a.out_cs + a.out_off + n] = v;
        }
    }
}

// [Cout][Cin][kh][kw] -> [K = (ky kw + kx) Cin + ci][npad], zero columns past Cout
__global__ void k_lfn_pack(const float *__restrict__ w, float *__restrict__ pk, int cout, int cin, int kh, int kw, int npad)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t K = (size_t)kh * kw * cin;
    if (t >= K * npad)
        return;
    const int n = (int)(t % npad), k = (int)(t / npad);
    const int tap = k / cin, ci = k - tap * cin, ky = tap / kw, kx = tap - ky * kw;
    pk[t] = n < cout ? w[(((size_t)n * cin + ci) * kh + ky) * kw + kx] : 0.f;
}

// ---- transposed conv, correlation, backwarp ------------------------------------------------------------------------

// ConvTranspose2d(C, C, 4, stride 2, padding 1, groups C, no bias): [n][h][w][C] -> [n][2h][2w][C]
__global__ void k_lfn_deconv(const float *__restrict__ in, const float *__restrict__ w, float *__restrict__ out, int h,
                             int wd, int C, size_t total)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total)
        return;
    const int c = (int)(t % C);
    const size_t p = t / C;
    const int W2 = 2 * wd, H2 = 2 * h;
    const int ox = (int)(p % W2), oy = (int)((p / W2) % H2);
    const size_t img = p / ((size_t)W2 * H2);
    const float *s = in + img * h * wd * C;
    const float *k = w + (size_t)c * 16;
    float acc = 0.f;
    const int iyh = (oy + 1) >> 1, ixh = (ox + 1) >> 1;
    for (int iy = iyh - 1; iy <= iyh; iy++) {
        const int ky = oy + 1 - 2 * iy;
        if (iy < 0 || iy >= h || ky < 0 || ky > 3)
            continue;
        for (int ix = ixh - 1; ix <= ixh; ix++) {
            const int kx = ox + 1 - 2 * ix;
            if (ix < 0 || ix >= wd || kx < 0 || kx > 3)
                continue;
            acc = acc + s[((size_t)iy * wd + ix) * C + c] * k[ky * 4 + kx];
        }
    }
    out[t] = acc;
}

// LeakyReLU(correlation): one lane per output position and displacement d.  Lane t of the CuPy kernel's 32 is the
// partial of the channels ch = t (mod 32), ascending, accumulated with an fma (NVRTC contracts `sum += a * b`); the
// partials are added in lane order to a total that starts at 0 and divided by (float)C.  Outside the frame the second
// operand is 0 (the kernel's zero padding).
__global__ void k_lfn_corr(const float *__restrict__ one, const float *__restrict__ two, float *__restrict__ out, int h,
                           int w, int C, int s, int ho, int wo, size_t total)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total)
        return;
    const int d = (int)(t % 49);
    const size_t p = t / 49;
    const int x = (int)(p % wo), y = (int)((p / wo) % ho);
    const size_t img = p / ((size_t)wo * ho);
    const int y1 = y * s, x1 = x * s, y2 = y1 + (d / 7 - 3) * s, x2 = x1 + (d % 7 - 3) * s;
    const float *a = one + ((img * h + y1) * w + x1) * C;
    const bool inside = y2 >= 0 && y2 < h && x2 >= 0 && x2 < w;
    const float *b = two + ((img * h + (inside ? y2 : 0)) * w + (inside ? x2 : 0)) * C;
    float total_sum = 0.f;
    for (int lane = 0; lane < 32; lane++) {
        float part = 0.f;
        for (int ch = lane; ch < C; ch += 32)
            part = __builtin_fmaf(a[ch], inside ? b[ch] : 0.f, part);
        total_sum = total_sum + part;
    }
    out[t] = lrelu(total_sum / (float)C);
}

// torch.linspace(-1, 1, n) in float32: -1 + step i below n / 2, 1 - step (n - 1 - i) from there
__device__ __forceinline__ float linspace_pm1(int i, int n)
{
    const float step = 2.0f / (float)(n - 1);
    return i < n / 2 ? -1.0f + step * (float)i : 1.0f - step * (float)(n - 1 - i);
}

struct Sample {
    int x0, y0;
    float nw, ne, sw, se;
    bool vx0, vx1, vy0, vy1;
};
// the bilinear sample grid_sample takes at pixel (x, y) for flow (u, v) scaled by `scale`
__device__ __forceinline__ Sample warp_sample(int x, int y, int w, int h, float u, float v, float scale)
{
    const float gx = linspace_pm1(x, w) + (u * scale) * (float)(2.0 / (w - 1.0));
    const float gy = linspace_pm1(y, h) + (v * scale) * (float)(2.0 / (h - 1.0));
    const float ix = ((gx + 1.f) / 2.f) * (float)(w - 1), iy = ((gy + 1.f) / 2.f) * (float)(h - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    Sample s;
    const bool fin = fx > -4.f && fx < (float)w + 4.f && fy > -4.f && fy < (float)h + 4.f; // (NaN: not finite)
    s.x0 = fin ? (int)fx : -8, s.y0 = fin ? (int)fy : -8;
    const float wx = ix - fx, wy = iy - fy, ex = 1.f - wx, sy = 1.f - wy;
    s.nw = sy * ex, s.ne = sy * wx, s.sw = wy * ex, s.se = wy * wx;
    s.vx0 = s.x0 >= 0 && s.x0 < w, s.vx1 = s.x0 + 1 >= 0 && s.x0 + 1 < w;
    s.vy0 = s.y0 >= 0 && s.y0 < h, s.vy1 = s.y0 + 1 >= 0 && s.y0 + 1 < h;
    return s;
}
__device__ __forceinline__ float warp_value(const float *img, int w, int C, int c, const Sample &s)
{
    const float a = s.vy0 && s.vx0 ? img[((size_t)s.y0 * w + s.x0) * C + c] : 0.f;
    const float b = s.vy0 && s.vx1 ? img[((size_t)s.y0 * w + s.x0 + 1) * C + c] : 0.f;
    const float d = s.vy1 && s.vx0 ? img[((size_t)(s.y0 + 1) * w + s.x0) * C + c] : 0.f;
    const float e = s.vy1 && s.vx1 ? img[((size_t)(s.y0 + 1) * w + s.x0 + 1) * C + c] : 0.f;
    return ((s.nw * a + s.ne * b) + s.sw * d) + s.se * e;
}

// backwarp(in, flow * scale): in [n][h][w][C] contiguous, flow [n][h][w][flow_cs] at flow_off, out [n][h][w][out_cs]
// at out_off
__global__ void k_lfn_backwarp(const float *__restrict__ in, int C, const float *__restrict__ flow, int flow_cs,
                               int flow_off, float scale, float *__restrict__ out, int out_cs, int out_off, int h, int w,
                               size_t total)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total)
        return;
    const int c = (int)(t % C);
    const size_t p = t / C;
    const int x = (int)(p % w), y = (int)((p / w) % h);
    const size_t img = p / ((size_t)w * h);
    const float *f = flow + p * flow_cs + flow_off;
    const Sample s = warp_sample(x, y, w, h, f[0], f[1], scale);
    out[p * out_cs + out_off + c] = warp_value(in + img * h * w * C, w, C, c, s);
}

// ---- Regularization -------------------------------------------------------------------------------------------------

// mean over the h x w pixels of flow channel c of image blockIdx.x: a strided sum per lane in double, then a fixed tree
__global__ __launch_bounds__(256) void k_lfn_mean(const float *__restrict__ flow, int npx, float *__restrict__ mean)
{
    __shared__ double red[256];
    const int img = blockIdx.x, c = blockIdx.y;
    const float *f = flow + (size_t)img * npx * 2 + c;
    double s = 0.0;
    for (int i = threadIdx.x; i < npx; i += 256)
        s += (double)f[(size_t)i * 2];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k)
            red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        mean[img * 2 + c] = (float)(red[0] / (double)npx);
}

// channels 0..2 of the Regularization concat: ||one - backwarp(two, flow * scale)||_2 over the 3 image channels, and
// flow - mean (images [n][h][w][3]: one = im, two = im + n h w 3)
__global__ void k_lfn_diff(const float *__restrict__ im1, const float *__restrict__ im2, const float *__restrict__ flow,
                           const float *__restrict__ mean, float scale, float *__restrict__ cat, int cat_cs, int h, int w,
                           size_t total)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total)
        return;
    const int x = (int)(p % w), y = (int)((p / w) % h);
    const size_t img = p / ((size_t)w * h);
    const float u = flow[p * 2], v = flow[p * 2 + 1];
    const Sample s = warp_sample(x, y, w, h, u, v, scale);
    const float *a = im1 + p * 3, *two = im2 + img * h * w * 3;
    float acc = 0.f;
    for (int c = 0; c < 3; c++) {
        const float d = a[c] - warp_value(two, w, 3, c, s);
        acc = acc + d * d;
    }
    float *o = cat + p * cat_cs;
    o[0] = sqrtf(acc);
    o[1] = u - mean[img * 2];
    o[2] = v - mean[img * 2 + 1];
}

// the end of the Regularization module, per pixel: e_c = exp(-d_c^2 - max_c(-d_c^2)); divisor = 1 / sum_c e_c;
// out_x = (sum_c wx_c (e_c ux_c) + bx) divisor with ux_c the flow's x at the c-th position of the k x k window (zero
// outside the frame), and the same for y
template <int K>
__global__ void k_lfn_tail(const float *__restrict__ dist, const float *__restrict__ flow, const float *__restrict__ wx,
                           const float *__restrict__ bx, const float *__restrict__ wy, const float *__restrict__ by,
                           float *__restrict__ out, int h, int w, size_t total)
{
    constexpr int K2 = K * K, R = (K - 1) / 2;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total)
        return;
    const int x = (int)(p % w), y = (int)((p / w) % h);
    const size_t img = p / ((size_t)w * h);
    const float *d = dist + p * K2;
    float mx = -INFINITY;
#pragma unroll 1
    for (int c = 0; c < K2; c++)
        mx = fmaxf(mx, -(d[c] * d[c]));
    // one pass for the sum of the e_c and the two weighted sums, each in ascending c (no array: nothing spills)
    const float *f = flow + img * h * w * 2;
    float sum = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll 1
    for (int dy = 0; dy < K; dy++) {
        const int yy = y + dy - R;
#pragma unroll
        for (int dx = 0; dx < K; dx++) {
            const int c = dy * K + dx, xx = x + dx - R;
            const float e = expf(-(d[c] * d[c]) - mx);
            sum = sum + e;
            float ux = 0.f, uy = 0.f;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w)
                ux = f[((size_t)yy * w + xx) * 2], uy = f[((size_t)yy * w + xx) * 2 + 1];
            sx = sx + wx[c] * (e * ux);
            sy = sy + wy[c] * (e * uy);
        }
    }
    const float div = 1.f / sum;
    out[p * 2] = (sx + bx[0]) * div;
    out[p * 2 + 1] = (sy + by[0]) * div;
}

// C channels of [n][h][w][C] into the slice at off of [n][h][w][cs]
__global__ void k_lfn_copy(const float *__restrict__ in, int C, float *__restrict__ out, int cs, int off, size_t total)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total)
        return;
    const size_t p = t / C;
    out[p * cs + off + (t % C)] = in[t];
}

} // namespace lfn
} // namespace tf

using namespace tf;
using namespace tf::lfn;

struct tf_lfn {
    int W, H, Wp, Hp, n_slots, max_pairs;
    Net net;
    bool has_weights = false;
    int precision = TF_LFN_F32;
    bool q_packed = false;          // qhi / qlo hold the current weights (repacked at the first call in a bf16 mode)
    DevBuf blob, packed, qhi, qlo, frames, bgr_stage;
    // activations, sized for max_pairs (features and images: 2 max_pairs frames, "one" frames first)
    DevBuf img[6], feat[6], bufA, bufB, bufFM, bufFS, bufW, cat, corr, corr2, flow_up, flow_s, flow_r, distA, distB,
        mean, out;
    int last_pairs = 0;
};

namespace {

const char *conv_label(int cls)
{
    static const char *names[CC_COUNT] = {"lfn_conv7x7",  "lfn_conv3x3_s1", "lfn_conv3x3_s2", "lfn_conv1x1",
                                          "lfn_conv_kx1", "lfn_conv_1xk",   "lfn_conv_head",  "lfn_conv_dist"};
    return names[cls];
}

// the labels of the bf16 kernel's launches that gather their input with 128-bit loads (tools/bench_lfn.py adds the two
// labels of a class; the precision tests read them to see which gather ran)
const char *conv_label_vec(int cls)
{
    static const char *names[CC_COUNT] = {"lfn_conv7x7_v",  "lfn_conv3x3_s1_v", "lfn_conv3x3_s2_v", "lfn_conv1x1_v",
                                          "lfn_conv_kx1_v", "lfn_conv_1xk_v",   "lfn_conv_head_v",  "lfn_conv_dist_v"};
    return names[cls];
}

// The bf16 weight planes of the bf16 and bf16x3 modes, made when a call first needs them and again after new weights.
int ensure_q_weights(tf_lfn *L)
{
    if (L->precision == TF_LFN_F32 || L->q_packed)
        return TF_OK;
    const size_t bytes = (size_t)L->net.q_elems * sizeof(uint16_t);
    if (!L->qhi.p)
        TF_TRY(L->qhi.alloc(bytes));
    if (!L->qlo.p)
        TF_TRY(L->qlo.alloc(bytes));
    for (const Layer &l : L->net.layers)
        if (!l.deconv)
            TF_TRY(pack_weights_q(l, L->blob.as<const float>() + l.w_off, L->qhi.as<uint16_t>() + l.q_off,
                                  L->qlo.as<uint16_t>() + l.q_off));
    L->q_packed = true;
    return TF_OK;
}

// One convolution over n images of hin x win.  Buffers are NHWC with the given channel strides and offsets.
int run_conv(tf_lfn *L, int li, int n, int hin, int win, const float *in, int in_cs, int in_off, float *out, int out_cs,
             int out_off, const float *res = nullptr, int res_cs = 0, int res_off = 0)
{
    const Layer &l = L->net.layers[li];
    ConvArgs a{};
    a.in = in, a.in_cs = in_cs, a.in_off = in_off;
    a.wt = L->packed.as<float>() + l.pk_off;
    a.bias = L->blob.as<float>() + l.b_off;
    a.out = out, a.out_cs = out_cs, a.out_off = out_off;
    a.res = res, a.res_cs = res_cs, a.res_off = res_off;
    a.hin = hin, a.win = win;
    a.ho = (hin + 2 * l.ph - l.kh) / l.stride + 1, a.wo = (win + 2 * l.pw - l.kw) / l.stride + 1;
    const long long M = (long long)n * a.ho * a.wo;
    TF_REQUIRE(M < (1ll << 31), "tf_lfn: %lld output pixels in one convolution", M);
    a.M = (int)M;
    a.cin = l.cin, a.cout = l.cout, a.kh = l.kh, a.kw = l.kw, a.stride = l.stride, a.ph = l.ph, a.pw = l.pw;
    a.K = l.kh * l.kw * l.cin, a.npad = l.npad, a.leaky = l.leaky;
    const char *name = conv_label(l.cls);
    if (L->precision != TF_LFN_F32)
        return launch_conv_q(name, conv_label_vec(l.cls), a, L->qhi.as<const uint16_t>() + l.q_off,
                             L->qlo.as<const uint16_t>() + l.q_off, l.kpad, l.nt, L->precision == TF_LFN_BF16 ? 1 : 3);
    const dim3 grid(cdiv(a.M, CONV_BM), l.npad / (32 * l.nt));
    switch (l.nt) {
    case 1: return launch(name, k_lfn_conv<1>, grid, dim3(CONV_THREADS), 0, a);
    case 2: return launch(name, k_lfn_conv<2>, grid, dim3(CONV_THREADS), 0, a);
    case 3: return launch(name, k_lfn_conv<3>, grid, dim3(CONV_THREADS), 0, a);
    default: return launch(name, k_lfn_conv<4>, grid, dim3(CONV_THREADS), 0, a);
    }
}

int run_deconv(tf_lfn *L, int li, int n, int h, int w, const float *in, float *out)
{
    const Layer &l = L->net.layers[li];
    const size_t total = (size_t)n * 4 * h * w * l.cout;
    return launch("lfn_deconv", k_lfn_deconv, dim3(cdiv(total, 256)), dim3(256), 0, in, L->blob.as<const float>() + l.w_off,
                  out, h, w, l.cout, total);
}

int run_corr(int n, int h, int w, int C, int s, const float *one, const float *two, float *out)
{
    const int ho = (h + s - 1) / s, wo = (w + s - 1) / s;
    const size_t total = (size_t)n * ho * wo * 49;
    return launch("lfn_corr", k_lfn_corr, dim3(cdiv(total, 256)), dim3(256), 0, one, two, out, h, w, C, s, ho, wo, total);
}

int run_backwarp(int n, int h, int w, int C, const float *in, const float *flow, int flow_cs, int flow_off, float scale,
                 float *out, int out_cs, int out_off)
{
    const size_t total = (size_t)n * h * w * C;
    return launch("lfn_backwarp", k_lfn_backwarp, dim3(cdiv(total, 256)), dim3(256), 0, in, C, flow, flow_cs, flow_off,
                  scale, out, out_cs, out_off, h, w, total);
}

int run_tail(tf_lfn *L, int level, int n, int h, int w, const float *dist, const float *flow, float *out)
{
    const LevelLayers &v = L->net.lv[level - 2];
    const float *B = L->blob.as<const float>();
    const Layer &lx = L->net.layers[v.r_scale_x], &ly = L->net.layers[v.r_scale_y];
    const size_t total = (size_t)n * h * w;
    const dim3 g(cdiv(total, 256)), b(256);
    const float *wx = B + lx.w_off, *bx = B + lx.b_off, *wy = B + ly.w_off, *by = B + ly.b_off;
    switch (UNFOLD[level]) {
    case 7: return launch("lfn_tail", k_lfn_tail<7>, g, b, 0, dist, flow, wx, bx, wy, by, out, h, w, total);
    case 5: return launch("lfn_tail", k_lfn_tail<5>, g, b, 0, dist, flow, wx, bx, wy, by, out, h, w, total);
    default: return launch("lfn_tail", k_lfn_tail<3>, g, b, 0, dist, flow, wx, bx, wy, by, out, h, w, total);
    }
}

int run_copy(int n, int h, int w, int C, const float *in, float *out, int cs, int off)
{
    const size_t total = (size_t)n * h * w * C;
    return launch("lfn_copy", k_lfn_copy, dim3(cdiv(total, 256)), dim3(256), 0, in, C, out, cs, off, total);
}

int run_prep(tf_lfn *L, int n_img, const int *slots, const int *roles, float *out)
{
    PrepArgs pa;
    std::memset(&pa, 0, sizeof pa);
    for (int i = 0; i < n_img; i++) {
        pa.src[i] = L->frames.as<const uint8_t>() + (size_t)slots[i] * L->W * L->H * 3;
        pa.role[i] = roles[i];
    }
    return launch("lfn_prep", k_lfn_prep, dim3(cdiv((size_t)L->Wp * L->Hp, 256), n_img), dim3(256), 0, pa, L->W, L->H, out,
                  L->Wp, L->Hp, (float)L->W / (float)L->Wp, (float)L->H / (float)L->Hp);
}

// The whole network for n pairs whose frames are already in their slots; flows into L->out.
int forward(tf_lfn *L, int n, const int *prev_slots, const int *next_slots)
{
    const Net &N = L->net;
    const int n2 = 2 * n;
    int slots[2 * MAX_PAIRS], roles[2 * MAX_PAIRS];
    for (int i = 0; i < n; i++) {
        slots[i] = prev_slots[i], roles[i] = 0;
        slots[n + i] = next_slots[i], roles[n + i] = 1;
    }
    TF_TRY(run_prep(L, n2, slots, roles, L->img[0].as<float>()));
    int hs[6], ws[6];
    for (int j = 0; j < 6; j++)
        hs[j] = L->Hp >> j, ws[j] = L->Wp >> j;
    for (int j = 1; j < 6; j++)
        TF_TRY(launch("lfn_pyramid", k_lfn_bilinear, dim3(cdiv((size_t)hs[j] * ws[j], 256), n2), dim3(256), 0,
                      L->img[j - 1].as<const float>(), 3, hs[j - 1], ws[j - 1], L->img[j].as<float>(), hs[j], ws[j],
                      (float)ws[j - 1] / (float)ws[j], (float)hs[j - 1] / (float)hs[j], 1.0f, 1.0f, 1.0f, 0));
    // feature pyramid over the 2n frames
    float *A = L->bufA.as<float>(), *B = L->bufB.as<float>();
    TF_TRY(run_conv(L, N.feat[0], n2, hs[0], ws[0], L->img[0].as<float>(), 3, 0, L->feat[0].as<float>(), 32, 0));
    TF_TRY(run_conv(L, N.feat[1], n2, hs[0], ws[0], L->feat[0].as<float>(), 32, 0, A, 32, 0));
    TF_TRY(run_conv(L, N.feat[2], n2, hs[1], ws[1], A, 32, 0, B, 32, 0));
    TF_TRY(run_conv(L, N.feat[3], n2, hs[1], ws[1], B, 32, 0, L->feat[1].as<float>(), 32, 0));
    TF_TRY(run_conv(L, N.feat[4], n2, hs[1], ws[1], L->feat[1].as<float>(), 32, 0, A, 64, 0));
    TF_TRY(run_conv(L, N.feat[5], n2, hs[2], ws[2], A, 64, 0, L->feat[2].as<float>(), 64, 0));
    TF_TRY(run_conv(L, N.feat[6], n2, hs[2], ws[2], L->feat[2].as<float>(), 64, 0, A, 96, 0));
    TF_TRY(run_conv(L, N.feat[7], n2, hs[3], ws[3], A, 96, 0, L->feat[3].as<float>(), 96, 0));
    TF_TRY(run_conv(L, N.feat[8], n2, hs[3], ws[3], L->feat[3].as<float>(), 96, 0, L->feat[4].as<float>(), 128, 0));
    TF_TRY(run_conv(L, N.feat[9], n2, hs[4], ws[4], L->feat[4].as<float>(), 128, 0, L->feat[5].as<float>(), 192, 0));

    float *cat = L->cat.as<float>(), *flow_up = L->flow_up.as<float>(), *flow_s = L->flow_s.as<float>();
    float *flow_r = L->flow_r.as<float>();
    for (int i = N_LEVELS - 1; i >= 0; i--) {
        const int lvl = i + 2, j = lvl - 1, h = hs[j], w = ws[j], C = FEAT_C[j];
        const size_t px = (size_t)n * h * w;
        const LevelLayers &v = N.lv[i];
        const float *f1 = L->feat[j].as<float>(), *f2 = f1 + px * C;
        const float scale = BACKWARP[lvl];
        // ---- Matching
        const float *m1 = f1, *m2 = f2;
        int Cm = C;
        if (v.m_feat >= 0) {
            TF_TRY(run_conv(L, v.m_feat, n2, h, w, f1, C, 0, L->bufFM.as<float>(), 64, 0));
            m1 = L->bufFM.as<float>(), m2 = m1 + px * 64, Cm = 64;
        }
        const bool first = lvl == 6;
        if (!first) {
            TF_TRY(run_deconv(L, v.m_upflow, n, h / 2, w / 2, flow_r, flow_up));
            TF_TRY(run_backwarp(n, h, w, Cm, m2, flow_up, 2, 0, scale, L->bufW.as<float>(), Cm, 0));
            m2 = L->bufW.as<float>();
        }
        if (lvl >= 4) {
            TF_TRY(run_corr(n, h, w, Cm, 1, m1, m2, L->corr.as<float>()));
        } else {
            TF_TRY(run_corr(n, h, w, Cm, 2, m1, m2, L->corr2.as<float>()));
            TF_TRY(run_deconv(L, v.m_upcorr, n, h / 2, w / 2, L->corr2.as<float>(), L->corr.as<float>()));
        }
        // the Subpixel concat [features one, warped features two, flow]: the Matching head writes the flow slice
        const int Cs = lvl == 2 ? 64 : C, scs = SUB_CIN[lvl];
        TF_TRY(run_conv(L, v.m_main[0], n, h, w, L->corr.as<float>(), 49, 0, A, 128, 0));
        TF_TRY(run_conv(L, v.m_main[1], n, h, w, A, 128, 0, B, 64, 0));
        TF_TRY(run_conv(L, v.m_main[2], n, h, w, B, 64, 0, A, 32, 0));
        TF_TRY(run_conv(L, v.m_main[3], n, h, w, A, 32, 0, cat, scs, 2 * Cs, first ? nullptr : flow_up, 2, 0));
        // ---- Subpixel
        const float *s2 = f2;
        if (v.s_feat >= 0) {
            TF_TRY(run_conv(L, v.s_feat, n, h, w, f1, C, 0, cat, scs, 0));
            TF_TRY(run_conv(L, v.s_feat, n, h, w, f2, C, 0, L->bufFS.as<float>(), 64, 0));
            s2 = L->bufFS.as<float>();
        } else {
            TF_TRY(run_copy(n, h, w, C, f1, cat, scs, 0));
        }
        TF_TRY(run_backwarp(n, h, w, Cs, s2, cat, scs, 2 * Cs, scale, cat, scs, Cs));
        TF_TRY(run_conv(L, v.s_main[0], n, h, w, cat, scs, 0, A, 128, 0));
        TF_TRY(run_conv(L, v.s_main[1], n, h, w, A, 128, 0, B, 64, 0));
        TF_TRY(run_conv(L, v.s_main[2], n, h, w, B, 64, 0, A, 32, 0));
        TF_TRY(run_conv(L, v.s_main[3], n, h, w, A, 32, 0, flow_s, 2, 0, cat, scs, 2 * Cs));
        // ---- Regularization: concat [difference, flow - mean, features]
        const int rcs = REG_CIN[lvl];
        TF_TRY(launch("lfn_mean", k_lfn_mean, dim3(n, 2), dim3(256), 0, (const float *)flow_s, h * w, L->mean.as<float>()));
        const float *im1 = L->img[j].as<float>(), *im2 = im1 + px * 3;
        TF_TRY(launch("lfn_diff", k_lfn_diff, dim3(cdiv(px, 256)), dim3(256), 0, im1, im2, (const float *)flow_s,
                      L->mean.as<const float>(), scale, cat, rcs, h, w, px));
        if (v.r_feat >= 0)
            TF_TRY(run_conv(L, v.r_feat, n, h, w, f1, C, 0, cat, rcs, 3));
        else
            TF_TRY(run_copy(n, h, w, C, f1, cat, rcs, 3));
        TF_TRY(run_conv(L, v.r_main[0], n, h, w, cat, rcs, 0, A, 128, 0));
        TF_TRY(run_conv(L, v.r_main[1], n, h, w, A, 128, 0, B, 128, 0));
        TF_TRY(run_conv(L, v.r_main[2], n, h, w, B, 128, 0, A, 64, 0));
        TF_TRY(run_conv(L, v.r_main[3], n, h, w, A, 64, 0, B, 64, 0));
        TF_TRY(run_conv(L, v.r_main[4], n, h, w, B, 64, 0, A, 32, 0));
        TF_TRY(run_conv(L, v.r_main[5], n, h, w, A, 32, 0, B, 32, 0));
        const int k2 = UNFOLD[lvl] * UNFOLD[lvl];
        float *dist = L->distB.as<float>();
        if (v.r_dist1 >= 0) {
            TF_TRY(run_conv(L, v.r_dist0, n, h, w, B, 32, 0, L->distA.as<float>(), k2, 0));
            TF_TRY(run_conv(L, v.r_dist1, n, h, w, L->distA.as<float>(), k2, 0, dist, k2, 0));
        } else {
            TF_TRY(run_conv(L, v.r_dist0, n, h, w, B, 32, 0, dist, k2, 0));
        }
        TF_TRY(run_tail(L, lvl, n, h, w, dist, flow_s, flow_r));
    }
    // x 20, bilinear to W x H, u x W / Wp, v x H / Hp
    return launch("lfn_output", k_lfn_bilinear, dim3(cdiv((size_t)L->W * L->H, 256), n), dim3(256), 0,
                  (const float *)flow_r, 2, hs[1], ws[1], L->out.as<float>(), L->H, L->W, (float)ws[1] / (float)L->W,
                  (float)hs[1] / (float)L->H, 20.0f, (float)((double)L->W / (double)L->Wp),
                  (float)((double)L->H / (double)L->Hp), 1);
}

int alloc_all(tf_lfn *L)
{
    const size_t n = L->max_pairs, n2 = 2 * n;
    size_t px[6];
    for (int j = 0; j < 6; j++)
        px[j] = (size_t)(L->Hp >> j) * (L->Wp >> j);
    const size_t F = sizeof(float);
    for (int j = 0; j < 6; j++) {
        TF_TRY(L->img[j].alloc(n2 * px[j] * 3 * F));
        TF_TRY(L->feat[j].alloc(n2 * px[j] * FEAT_C[j] * F));
    }
    const size_t m2 = px[1]; // level 2
    TF_TRY(L->bufA.alloc(n * m2 * 128 * F));
    TF_TRY(L->bufB.alloc(n * m2 * 128 * F));
    TF_TRY(L->bufFM.alloc(n2 * m2 * 64 * F));
    TF_TRY(L->bufFS.alloc(n * m2 * 64 * F));
    TF_TRY(L->bufW.alloc(n * m2 * 64 * F));
    TF_TRY(L->cat.alloc(n * m2 * 131 * F));
    TF_TRY(L->corr.alloc(n * m2 * 49 * F));
    TF_TRY(L->corr2.alloc(n * (m2 / 4) * 49 * F));
    TF_TRY(L->flow_up.alloc(n * m2 * 2 * F));
    TF_TRY(L->flow_s.alloc(n * m2 * 2 * F));
    TF_TRY(L->flow_r.alloc(n * m2 * 2 * F));
    TF_TRY(L->distA.alloc(n * m2 * 49 * F));
    TF_TRY(L->distB.alloc(n * m2 * 49 * F));
    TF_TRY(L->mean.alloc(n * 2 * F));
    TF_TRY(L->out.alloc(n * L->W * L->H * 2 * F));
    return TF_OK;
}

// a temporary device copy of a host array
int upload(DevBuf &d, const void *host, size_t bytes)
{
    TF_TRY(d.alloc(bytes ? bytes : 4));
    if (bytes)
        TF_HIP(hipMemcpyAsync(d.p, host, bytes, hipMemcpyHostToDevice, stream()));
    return TF_OK;
}

int download(void *host, const DevBuf &d, size_t bytes)
{
    TF_HIP(hipMemcpyAsync(host, d.p, bytes, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

} // namespace

TF_API int tf_lfn_create(tf_lfn **out, int width, int height, int frame_slots, int max_pairs)
{
    TF_REQUIRE(out, "tf_lfn_create: null pointer");
    *out = nullptr;
    // at 32 px or less in a dimension the network's 1/32 level is 1 px wide and the reference's backwarp divides by
    // zero (2.0 / (size - 1.0) raises ZeroDivisionError)
    TF_REQUIRE(width > 32 && height > 32 && width < 32768 && height < 32768,
               "tf_lfn_create: size %dx%d (LiteFlowNet needs more than 32 px in each dimension: the reference raises "
               "ZeroDivisionError below)", width, height);
    TF_REQUIRE(frame_slots >= 2, "tf_lfn_create: frame_slots %d < 2", frame_slots);
    TF_REQUIRE(max_pairs >= 1 && max_pairs <= MAX_PAIRS, "tf_lfn_create: max_pairs %d not in [1, %d]", max_pairs, MAX_PAIRS);
    TF_TRY(ensure_init());
    auto L = make_handle<tf_lfn>();
    TF_REQUIRE(L, "tf_lfn_create: out of memory");
    L->W = width, L->H = height, L->n_slots = frame_slots, L->max_pairs = max_pairs;
    L->Wp = (width + 31) / 32 * 32, L->Hp = (height + 31) / 32 * 32;
    L->net = make_net();
    TF_TRY(L->frames.alloc((size_t)frame_slots * width * height * 3));
    TF_TRY(alloc_all(L.get()));
    *out = L.release();
    return TF_OK;
}

TF_API void tf_lfn_destroy(tf_lfn *lfn)
{
    if (lfn)
        (void)hipStreamSynchronize(stream()); // kernels of the handle's last call may still read its buffers
    delete lfn;
}

TF_API int tf_lfn_set_weights(tf_lfn *L, const float *blob, long long n_floats)
{
    TF_REQUIRE(L && blob, "tf_lfn_set_weights: null pointer");
    TF_REQUIRE(n_floats == L->net.blob_floats, "tf_lfn_set_weights: %lld floats, the network has %lld", n_floats,
               L->net.blob_floats);
    L->has_weights = false;
    L->q_packed = false;
    if (!L->blob.p)
        TF_TRY(L->blob.alloc((size_t)n_floats * sizeof(float)));
    if (!L->packed.p)
        TF_TRY(L->packed.alloc((size_t)L->net.packed_floats * sizeof(float)));
    TF_HIP(hipMemcpyAsync(L->blob.p, blob, (size_t)n_floats * sizeof(float), hipMemcpyHostToDevice, stream()));
    for (const Layer &l : L->net.layers) {
        if (l.deconv)
            continue;
        const size_t total = (size_t)l.kh * l.kw * l.cin * l.npad;
        TF_TRY(launch("lfn_pack", k_lfn_pack, dim3(cdiv(total, 256)), dim3(256), 0, L->blob.as<const float>() + l.w_off,
                      L->packed.as<float>() + l.pk_off, l.cout, l.cin, l.kh, l.kw, l.npad));
    }
    TF_HIP(hipStreamSynchronize(stream())); // the host blob is borrowed for this call only
    L->has_weights = true;
    return TF_OK;
}

TF_API int tf_lfn_set_precision(tf_lfn *L, int precision)
{
    TF_REQUIRE(L, "tf_lfn_set_precision: null pointer");
    TF_REQUIRE(precision == TF_LFN_F32 || precision == TF_LFN_BF16 || precision == TF_LFN_BF16X3,
               "tf_lfn_set_precision: %d is not TF_LFN_F32, TF_LFN_BF16 or TF_LFN_BF16X3", precision);
    L->precision = precision;
    return TF_OK;
}

TF_API int tf_lfn_get_precision(tf_lfn *L, int *precision)
{
    TF_REQUIRE(L && precision, "tf_lfn_get_precision: null pointer");
    *precision = L->precision;
    return TF_OK;
}

TF_API int tf_lfn_set_frame_bgr(tf_lfn *L, int slot, const uint8_t *bgr, int src_width, int src_height, ptrdiff_t stride)
{
    TF_REQUIRE(L && bgr, "tf_lfn_set_frame_bgr: null pointer");
    TF_REQUIRE(slot >= 0 && slot < L->n_slots, "tf_lfn_set_frame_bgr: slot %d out of range (%d slots)", slot, L->n_slots);
    TF_REQUIRE(src_width >= 1 && src_height >= 1 && (long long)src_width * src_height < (1ll << 31),
               "tf_lfn_set_frame_bgr: bad source size %dx%d", src_width, src_height);
    TF_REQUIRE(stride >= (ptrdiff_t)3 * src_width, "tf_lfn_set_frame_bgr: stride %td smaller than a row of %d BGR pixels",
               stride, src_width);
    const size_t row = (size_t)3 * src_width, need = row * src_height;
    if (L->bgr_stage.bytes < need) {
        TF_HIP(hipStreamSynchronize(stream()));
        L->bgr_stage.release();
        TF_TRY(L->bgr_stage.alloc(need));
    }
    uint8_t *dst = L->frames.as<uint8_t>() + (size_t)slot * L->W * L->H * 3;
    TF_HIP(hipMemcpy2DAsync(L->bgr_stage.p, row, bgr, (size_t)stride, row, src_height, hipMemcpyHostToDevice, stream()));
    const size_t npx = (size_t)L->W * L->H;
    TF_TRY(launch("lfn_ingest", k_lfn_ingest, dim3(cdiv(npx, 256)), dim3(256), 0, L->bgr_stage.as<const uint8_t>(), src_width,
                  src_height, dst, L->W, L->H, 1.0 / ((double)L->W / src_width), 1.0 / ((double)L->H / src_height)));
    TF_HIP(hipStreamSynchronize(stream())); // the host frame is borrowed for this call only
    return TF_OK;
}

TF_API int tf_lfn_calc_slots(tf_lfn *L, int n_pairs, const int *prev_slots, const int *next_slots)
{
    TF_REQUIRE(L && prev_slots && next_slots, "tf_lfn_calc_slots: null pointer");
    TF_REQUIRE(n_pairs >= 1 && n_pairs <= L->max_pairs, "tf_lfn_calc_slots: %d pairs (handle takes 1..%d)", n_pairs,
               L->max_pairs);
    TF_REQUIRE(L->has_weights, "tf_lfn_calc_slots: no weights (tf_lfn_set_weights)");
    for (int i = 0; i < n_pairs; i++)
        TF_REQUIRE(prev_slots[i] >= 0 && prev_slots[i] < L->n_slots && next_slots[i] >= 0 && next_slots[i] < L->n_slots,
                   "tf_lfn_calc_slots: pair %d: slots (%d, %d) out of range (%d slots)", i, prev_slots[i], next_slots[i],
                   L->n_slots);
    L->last_pairs = 0;
    TF_TRY(ensure_q_weights(L));
    TF_TRY(forward(L, n_pairs, prev_slots, next_slots));
    L->last_pairs = n_pairs;
    return TF_OK;
}

TF_API int tf_lfn_get_flow(tf_lfn *L, int pair, float *flow_out)
{
    TF_REQUIRE(L && flow_out, "tf_lfn_get_flow: null pointer");
    TF_REQUIRE(pair >= 0 && pair < L->last_pairs, "tf_lfn_get_flow: pair %d was not computed by the last call", pair);
    const size_t bytes = (size_t)L->W * L->H * 2 * sizeof(float);
    TF_HIP(hipMemcpyAsync(flow_out, (char *)L->out.p + (size_t)pair * bytes, bytes, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

TF_API int tf_lfn_flow_ptr(tf_lfn *L, int pair, void **dev)
{
    TF_REQUIRE(L && dev, "tf_lfn_flow_ptr: null pointer");
    TF_REQUIRE(pair >= 0 && pair < L->last_pairs, "tf_lfn_flow_ptr: pair %d was not computed by the last call", pair);
    *dev = (char *)L->out.p + (size_t)pair * L->W * L->H * 2 * sizeof(float);
    return TF_OK;
}

// ---- stage entry points (tests): host arrays in and out, through temporary device buffers ----------------------------

TF_API int tf_lfn_stage_conv(tf_lfn *L, int layer, int n, int h, int w, const float *in, int in_cs, int in_off,
                             const float *res, int res_cs, int res_off, float *out, int out_cs, int out_off)
{
    TF_REQUIRE(L && in && out, "tf_lfn_stage_conv: null pointer");
    TF_REQUIRE(L->has_weights, "tf_lfn_stage_conv: no weights");
    TF_REQUIRE(layer >= 0 && layer < (int)L->net.layers.size() && !L->net.layers[layer].deconv,
               "tf_lfn_stage_conv: %d is not a convolution", layer);
    const Layer &l = L->net.layers[layer];
    TF_REQUIRE(n >= 1 && h >= 1 && w >= 1 && (long long)n * h * w < (1ll << 28), "tf_lfn_stage_conv: bad size");
    TF_REQUIRE(in_off >= 0 && in_off + l.cin <= in_cs, "tf_lfn_stage_conv: input slice [%d, %d) of %d channels", in_off,
               in_off + l.cin, in_cs);
    TF_REQUIRE(out_off >= 0 && out_off + l.cout <= out_cs, "tf_lfn_stage_conv: output slice [%d, %d) of %d channels",
               out_off, out_off + l.cout, out_cs);
    TF_REQUIRE(!res || (res_off >= 0 && res_off + l.cout <= res_cs), "tf_lfn_stage_conv: residual slice out of range");
    const int ho = (h + 2 * l.ph - l.kh) / l.stride + 1, wo = (w + 2 * l.pw - l.kw) / l.stride + 1;
    TF_REQUIRE(ho >= 1 && wo >= 1, "tf_lfn_stage_conv: empty output");
    const size_t nin = (size_t)n * h * w * in_cs, nout = (size_t)n * ho * wo * out_cs, nres = res ? (size_t)n * ho * wo * res_cs : 0;
    DevBuf di, dout, dres;
    TF_TRY(upload(di, in, nin * 4));
    TF_TRY(upload(dout, out, nout * 4));
    if (res)
        TF_TRY(upload(dres, res, nres * 4));
    TF_TRY(ensure_q_weights(L));
    TF_TRY(run_conv(L, layer, n, h, w, di.as<float>(), in_cs, in_off, dout.as<float>(), out_cs, out_off,
                    res ? dres.as<float>() : nullptr, res_cs, res_off));
    return download(out, dout, nout * 4);
}

TF_API int tf_lfn_stage_deconv(tf_lfn *L, int layer, int n, int h, int w, const float *in, float *out)
{
    TF_REQUIRE(L && in && out, "tf_lfn_stage_deconv: null pointer");
    TF_REQUIRE(L->has_weights, "tf_lfn_stage_deconv: no weights");
    TF_REQUIRE(layer >= 0 && layer < (int)L->net.layers.size() && L->net.layers[layer].deconv,
               "tf_lfn_stage_deconv: %d is not a transposed convolution", layer);
    TF_REQUIRE(n >= 1 && h >= 1 && w >= 1 && (long long)n * h * w < (1ll << 26), "tf_lfn_stage_deconv: bad size");
    const int C = L->net.layers[layer].cout;
    DevBuf di, dout;
    TF_TRY(upload(di, in, (size_t)n * h * w * C * 4));
    TF_TRY(dout.alloc((size_t)n * 4 * h * w * C * 4));
    TF_TRY(run_deconv(L, layer, n, h, w, di.as<float>(), dout.as<float>()));
    return download(out, dout, (size_t)n * 4 * h * w * C * 4);
}

TF_API int tf_lfn_stage_correlation(tf_lfn *L, int stride, int n, int h, int w, int c, const float *one, const float *two,
                                    float *out)
{
    TF_REQUIRE(L && one && two && out, "tf_lfn_stage_correlation: null pointer");
    TF_REQUIRE(stride == 1 || stride == 2, "tf_lfn_stage_correlation: stride %d", stride);
    TF_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 1 && (long long)n * h * w * c < (1ll << 28),
               "tf_lfn_stage_correlation: bad size");
    const size_t nin = (size_t)n * h * w * c;
    const size_t nout = (size_t)n * ((h + stride - 1) / stride) * ((w + stride - 1) / stride) * 49;
    DevBuf d1, d2, dout;
    TF_TRY(upload(d1, one, nin * 4));
    TF_TRY(upload(d2, two, nin * 4));
    TF_TRY(dout.alloc(nout * 4));
    TF_TRY(run_corr(n, h, w, c, stride, d1.as<float>(), d2.as<float>(), dout.as<float>()));
    return download(out, dout, nout * 4);
}

TF_API int tf_lfn_stage_backwarp(tf_lfn *L, int n, int h, int w, int c, const float *in, const float *flow, float scale,
                                 float *out)
{
    TF_REQUIRE(L && in && flow && out, "tf_lfn_stage_backwarp: null pointer");
    TF_REQUIRE(n >= 1 && h >= 2 && w >= 2 && c >= 1 && (long long)n * h * w * c < (1ll << 28),
               "tf_lfn_stage_backwarp: bad size (at least 2 x 2)");
    const size_t nin = (size_t)n * h * w * c, nf = (size_t)n * h * w * 2;
    DevBuf di, df, dout;
    TF_TRY(upload(di, in, nin * 4));
    TF_TRY(upload(df, flow, nf * 4));
    TF_TRY(dout.alloc(nin * 4));
    TF_TRY(run_backwarp(n, h, w, c, di.as<float>(), df.as<float>(), 2, 0, scale, dout.as<float>(), c, 0));
    return download(out, dout, nin * 4);
}

TF_API int tf_lfn_stage_regularize_tail(tf_lfn *L, int level, int n, int h, int w, const float *dist, const float *flow,
                                        float *out)
{
    TF_REQUIRE(L && dist && flow && out, "tf_lfn_stage_regularize_tail: null pointer");
    TF_REQUIRE(L->has_weights, "tf_lfn_stage_regularize_tail: no weights");
    TF_REQUIRE(level >= 2 && level <= 6, "tf_lfn_stage_regularize_tail: level %d not in [2, 6]", level);
    TF_REQUIRE(n >= 1 && h >= 1 && w >= 1 && (long long)n * h * w < (1ll << 24), "tf_lfn_stage_regularize_tail: bad size");
    const int k2 = UNFOLD[level] * UNFOLD[level];
    const size_t px = (size_t)n * h * w;
    DevBuf dd, df, dout;
    TF_TRY(upload(dd, dist, px * k2 * 4));
    TF_TRY(upload(df, flow, px * 2 * 4));
    TF_TRY(dout.alloc(px * 2 * 4));
    TF_TRY(run_tail(L, level, n, h, w, dd.as<float>(), df.as<float>(), dout.as<float>()));
    return download(out, dout, px * 2 * 4);
}

TF_API int tf_lfn_stage_prep(tf_lfn *L, int slot, int role, float *out)
{
    TF_REQUIRE(L && out, "tf_lfn_stage_prep: null pointer");
    TF_REQUIRE(slot >= 0 && slot < L->n_slots, "tf_lfn_stage_prep: slot %d out of range", slot);
    TF_REQUIRE(role == 0 || role == 1, "tf_lfn_stage_prep: role %d (0 one, 1 two)", role);
    const size_t bytes = (size_t)L->Wp * L->Hp * 3 * 4;
    DevBuf d;
    TF_TRY(d.alloc(bytes));
    TF_TRY(run_prep(L, 1, &slot, &role, d.as<float>()));
    return download(out, d, bytes);
}
