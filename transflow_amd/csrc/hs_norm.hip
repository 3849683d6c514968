// The convergence test of Horn-Schunck, `numpy.linalg.norm(u - prev, 2) < delta`: the spectral norm sigma of du.
// Decided on the device when it can be, with a relative guard g = GUARD that covers LAPACK's own rounding of sigma:
//   1. cheap bounds from the iteration kernel's partial sums: F = ||du||_F >= sigma, U = sqrt(||du||_1 ||du||_inf) >= sigma,
//      L = max(largest column norm, largest row norm) <= sigma.  Converged if min(F, U) < delta (1 - g), not converged if
//      L >= delta (1 + g).
//   2. power iteration on du (du computed on the fly from the two u buffers, from the ones vector): ||du x|| / ||x||
//      is a lower bound; not converged once it reaches delta (1 + g).
//   3. Gram certificate: G = A A^T on the smaller side, A = du / F, in float64; sigma <= F ||G^k||_F^(1 / (2k)) for
//      k = 1, 2, 4.  Converged once that is below delta (1 - g).
//   4. otherwise (sigma within the guard of delta, or du not finite) the host evaluates the reference's expression.
// Every sum runs in a fixed order (no atomics): the same field gets the same decision every time.
#include "hs_common.h"

#include <limits>

namespace tf {
namespace hs {

constexpr int PW_CHUNKS = 32;   // row chunks of the du^T y product

int NormScratch::init(int w, int h)
{
    W = w, H = h;
    TF_TRY(partials.alloc(partial_doubles(w, h) * sizeof(double)));
    TF_TRY(blocks.alloc((size_t)n_bound_blocks(w, h) * 4 * sizeof(double)));
    TF_TRY(pw_x.alloc((size_t)w * sizeof(double)));
    TF_TRY(pw_y.alloc((size_t)h * sizeof(double)));
    TF_TRY(pw_xpart.alloc((size_t)PW_CHUNKS * w * sizeof(double)));
    TF_TRY(pw_scal.alloc((2 + 2 * POWER_STEPS) * sizeof(double)));
    TF_TRY(sums.alloc(256 * sizeof(double)));
    host_blocks.resize((size_t)n_bound_blocks(w, h) * 4);
    return TF_OK;
}

template <typename T> __device__ __forceinline__ double delta_at(const T *un, const T *uo, size_t i)
{
    return (double)(T)(un[i] - uo[i]);
}

// the cheap bounds' partials of du alone: the iteration kernel's strip walk without the iteration
template <typename T>
__global__ __launch_bounds__(IT_BX) void k_hs_delta_partials(const T *__restrict__ un, const T *__restrict__ uo, int W, int H,
                                                             double *__restrict__ P)
{
    __shared__ double rowred[IT_ROWS][4][2];
    const int c0 = blockIdx.x * IT_BX + threadIdx.x;
    const bool valid = c0 < W;
    const int c = valid ? c0 : W - 1;
    const int r0 = blockIdx.y * IT_ROWS, r1 = min(r0 + IT_ROWS, H);
    double csq = 0.0, cab = 0.0;
    for (int r = r0; r < r1; r++) {
        const double dd = valid ? delta_at(un, uo, (size_t)r * W + c) : 0.0;
        const double sq = dd * dd, ab = fabs(dd);
        csq = csq + sq;
        cab = cab + ab;
        const double wsq = wave_sum(sq), wab = wave_sum(ab);
        if ((threadIdx.x & 63) == 0) {
            rowred[r - r0][threadIdx.x >> 6][0] = wsq;
            rowred[r - r0][threadIdx.x >> 6][1] = wab;
        }
    }
    strip_store(P, W, H, valid ? c0 : -1, blockIdx.y, blockIdx.x, r0, r1 - r0, csq, cab, rowred);
}

// Block b < ceil(W / 256): 256 columns, each the sum of its strips' partials; else 256 rows, each the sum of its column
// blocks'.  Out: {max sum of du^2, max sum of |du|, sum of du^2 (column blocks only), number of non-finite sums}.
__global__ __launch_bounds__(256) void k_hs_bounds_reduce(const double *__restrict__ partials, size_t stride, PairList pl, int W,
                                                          int H, double *__restrict__ out)
{
    __shared__ double red[4][256];
    const int pair = pl.p[blockIdx.y].pair;
    const double *P = partials + (size_t)pair * stride;
    const int S = n_strips(H), CB = n_colblocks(W), ncbw = (W + 255) / 256, t = threadIdx.x;
    double sq = 0.0, ab = 0.0;
    bool in = false;
    if ((int)blockIdx.x < ncbw) {
        const int c = blockIdx.x * 256 + t;
        if (c < W) {
            in = true;
            for (int s = 0; s < S; s++) {
                sq = sq + P[(size_t)s * W + c];
                ab = ab + P[(size_t)S * W + (size_t)s * W + c];
            }
        }
    } else {
        const int r = (blockIdx.x - ncbw) * 256 + t;
        if (r < H) {
            in = true;
            const double *R = P + 2 * (size_t)S * W;
            for (int b = 0; b < CB; b++) {
                sq = sq + R[(size_t)b * H + r];
                ab = ab + R[(size_t)CB * H + (size_t)b * H + r];
            }
        }
    }
    const bool fin = isfinite(sq) && isfinite(ab);
    red[0][t] = in && fin ? sq : 0.0;
    red[1][t] = in && fin ? ab : 0.0;
    red[2][t] = in && fin && (int)blockIdx.x < ncbw ? sq : 0.0;
    red[3][t] = in && !fin ? 1.0 : 0.0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            red[0][t] = fmax(red[0][t], red[0][t + o]);
            red[1][t] = fmax(red[1][t], red[1][t + o]);
            red[2][t] = red[2][t] + red[2][t + o];
            red[3][t] = red[3][t] + red[3][t + o];
        }
        __syncthreads();
    }
    if (t < 4)
        out[((size_t)pair * gridDim.x + blockIdx.x) * 4 + t] = red[t][0];
}

int launch_bounds_reduce(const double *partials_base, size_t partials_stride, const PairList &pl, int W, int H, double *blocks_out)
{
    return launch("hs_bounds", k_hs_bounds_reduce, dim3(n_bound_blocks(W, H), pl.n), dim3(256), 0, partials_base, partials_stride,
                  pl, W, H, blocks_out);
}

int launch_delta_partials(const void *u_new, const void *u_old, bool f64, int W, int H, double *partials)
{
    const dim3 grid(n_colblocks(W), n_strips(H));
    if (f64)
        return launch("hs_delta_partials", k_hs_delta_partials<double>, grid, dim3(IT_BX), 0, (const double *)u_new,
                      (const double *)u_old, W, H, partials);
    return launch("hs_delta_partials", k_hs_delta_partials<float>, grid, dim3(IT_BX), 0, (const float *)u_new,
                  (const float *)u_old, W, H, partials);
}

template <typename T> __global__ void k_hs_delta(const T *__restrict__ un, const T *__restrict__ uo, T *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        out[i] = un[i] - uo[i];
}

int launch_delta(const void *u_new, const void *u_old, bool f64, size_t n, void *dst)
{
    if (f64)
        return launch("hs_delta", k_hs_delta<double>, dim3(cdiv(n, 256)), dim3(256), 0, (const double *)u_new,
                      (const double *)u_old, (double *)dst, n);
    return launch("hs_delta", k_hs_delta<float>, dim3(cdiv(n, 256)), dim3(256), 0, (const float *)u_new, (const float *)u_old,
                  (float *)dst, n);
}

Bounds bounds_of(const double *blocks, int W, int H)
{
    const int ncbw = (W + 255) / 256, nb = n_bound_blocks(W, H);
    double F2 = 0.0, L2 = 0.0, n1 = 0.0, ninf = 0.0, bad = 0.0;
    for (int b = 0; b < nb; b++) {
        const double *q = blocks + (size_t)b * 4;
        L2 = q[0] > L2 ? q[0] : L2;
        if (b < ncbw) {
            n1 = q[1] > n1 ? q[1] : n1;
            F2 += q[2];
        } else {
            ninf = q[1] > ninf ? q[1] : ninf;
        }
        bad += q[3];
    }
    Bounds r;
    r.nonfinite = bad > 0 || !std::isfinite(F2) || !std::isfinite(n1 * ninf);
    // A square of du that is denormal or flushed to zero is wrong by up to 2^-1075: at most 2^-1044 over W * H < 2^31
    // values.  From TINY_F2 up that is nothing beside a sum of squares that decides wrongly: such a sum is compared
    // with a delta^2 near sigma^2 >= F^2 / min(W, H) > 2^-976.  Below it the squares cannot be trusted.
    r.tiny = !r.nonfinite && F2 < TINY_F2;
    r.F = std::sqrt(F2);
    r.L = std::sqrt(L2);
    r.U = r.tiny ? std::sqrt(n1) * std::sqrt(ninf) : std::sqrt(n1 * ninf);   // (the product underflows with the squares)
    return r;
}

int decide_bounds(const Bounds &b, double delta)
{
    if (b.nonfinite)
        return UNDECIDED;        // NaN: numpy.linalg.norm raises; inf: it returns nan.  The host's call says which.
    if (!(delta > 0))
        return NOT_CONVERGED;    // sigma >= 0 is never below it
    if (b.tiny) {                // F and L lost squares: U alone (zero, or normal: a denormal U is itself rounded coarsely),
        const bool usable = b.U == 0 || b.U >= std::numeric_limits<double>::min();
        return usable && b.U < delta * (1 - GUARD) ? CONVERGED : UNDECIDED;   // and it can only say CONVERGED
    }
    if ((b.F < b.U ? b.F : b.U) < delta * (1 - GUARD))
        return CONVERGED;
    if (b.L >= delta * (1 + GUARD))
        return NOT_CONVERGED;
    return UNDECIDED;
}

// ---- power iteration --------------------------------------------------------------------------------------------
__global__ void k_fill(double *x, int n, double v)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        x[i] = v;
}

// one block: s = ||x||; scal[0] = 1 / s (0 for a zero vector); lb (if not null) = s
__global__ __launch_bounds__(1024) void k_norm(const double *__restrict__ x, int n, double *__restrict__ inv, double *__restrict__ lb)
{
    __shared__ double red[1024];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += 1024)
        s = s + x[i] * x[i];
    red[t] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o)
            red[t] = red[t] + red[t + o];
        __syncthreads();
    }
    if (t == 0) {
        const double nrm = sqrt(red[0]);
        *inv = nrm > 0 ? 1.0 / nrm : 0.0;
        if (lb)
            *lb = nrm;
    }
}

// y[i] = (sum_j du[i][j] x[j]) * inv_x: a block per row
template <typename T>
__global__ __launch_bounds__(256) void k_pw_rows(const T *__restrict__ un, const T *__restrict__ uo, int W,
                                                 const double *__restrict__ x, const double *__restrict__ inv_x, double *__restrict__ y)
{
    __shared__ double red[256];
    const int t = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * W;
    double s = 0.0;
    for (int j = t; j < W; j += 256)
        s = s + delta_at(un, uo, row + j) * x[j];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o)
            red[t] = red[t] + red[t + o];
        __syncthreads();
    }
    if (t == 0)
        y[blockIdx.x] = red[0] * *inv_x;
}

// xpart[chunk][j] = (sum over the chunk's rows i of du[i][j] y[i]) * inv_y
template <typename T>
__global__ __launch_bounds__(256) void k_pw_cols(const T *__restrict__ un, const T *__restrict__ uo, int W, int H,
                                                 const double *__restrict__ y, const double *__restrict__ inv_y,
                                                 double *__restrict__ xpart)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= W)
        return;
    const int rows = (H + PW_CHUNKS - 1) / PW_CHUNKS, i0 = blockIdx.y * rows, i1 = min(i0 + rows, H);
    double s = 0.0;
    for (int i = i0; i < i1; i++)
        s = s + delta_at(un, uo, (size_t)i * W + j) * y[i];
    xpart[(size_t)blockIdx.y * W + j] = s * *inv_y;
}

__global__ void k_pw_combine(const double *__restrict__ xpart, int W, double *__restrict__ x)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= W)
        return;
    double s = 0.0;
    for (int c = 0; c < PW_CHUNKS; c++)
        s = s + xpart[(size_t)c * W + j];
    x[j] = s;
}

// ---- Gram certificate -----------------------------------------------------------------------------------------
// A = du / F on the smaller side: [p][m] with p = min(H, W) rows
template <typename T>
__global__ void k_gram_build(const T *__restrict__ un, const T *__restrict__ uo, int W, int H, double invF, double *__restrict__ A)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)W * H)
        return;
    const double d = delta_at(un, uo, i) * invF;
    const size_t r = i / W, c = i % W;
    if (H <= W)
        A[i] = d;
    else
        A[c * H + r] = d;
}

// C = A A^T, A [p][m] row-major: 64 x 64 tiles, 4 x 4 per thread, 16-deep slices of A through LDS
__global__ __launch_bounds__(256) void k_syrk(const double *__restrict__ A, int p, int m, double *__restrict__ C)
{
    __shared__ double As[16][65], Bs[16][65];
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    double acc[4][4] = {};
    for (int k0 = 0; k0 < m; k0 += 16) {
        for (int e = t; e < 64 * 16; e += 256) {
            const int r = e / 16, kk = e % 16, k = k0 + kk;
            As[kk][r] = (i0 + r < p && k < m) ? A[(size_t)(i0 + r) * m + k] : 0.0;
            Bs[kk][r] = (j0 + r < p && k < m) ? A[(size_t)(j0 + r) * m + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                a[q] = As[kk][ty + 16 * q];
                b[q] = Bs[kk][tx + 16 * q];
            }
#pragma unroll
            for (int qa = 0; qa < 4; qa++)
#pragma unroll
                for (int qb = 0; qb < 4; qb++)
                    acc[qa][qb] = fma(a[qa], b[qb], acc[qa][qb]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int qa = 0; qa < 4; qa++)
#pragma unroll
        for (int qb = 0; qb < 4; qb++) {
            const int i = i0 + ty + 16 * qa, j = j0 + tx + 16 * qb;
            if (i < p && j < p)
                C[(size_t)i * p + j] = acc[qa][qb];
        }
}

// 256 blocks of partial sums of squares (the host adds them in order)
__global__ __launch_bounds__(256) void k_sumsq(const double *__restrict__ x, size_t n, double *__restrict__ out)
{
    __shared__ double red[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + t; i < n; i += (size_t)256 * gridDim.x)
        s = s + x[i] * x[i];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o)
            red[t] = red[t] + red[t + o];
        __syncthreads();
    }
    if (t == 0)
        out[blockIdx.x] = red[0];
}

static int frobenius(NormScratch &s, const double *x, size_t n, double *out)
{
    TF_TRY(launch("hs_gram_norm", k_sumsq, dim3(256), dim3(256), 0, x, n, s.sums.as<double>()));
    double h[256];
    TF_HIP(hipMemcpyAsync(h, s.sums.p, sizeof h, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    double t = 0.0;
    for (double v : h)
        t += v;
    *out = std::sqrt(t);
    return TF_OK;
}

static_assert(POWER_STEPS % 2 == 0, "the power bounds are read back after every second step");

// ---- the stages' steps: what decide_device and device_values both run ----------------------------------------
// power iteration: x = the normalised ones vector
static int power_start(NormScratch &s)
{
    double *x = s.pw_x.as<double>(), *scal = s.pw_scal.as<double>();
    TF_TRY(launch("hs_power", k_fill, dim3(cdiv(s.W, 256)), dim3(256), 0, x, s.W, 1.0));
    return launch("hs_power", k_norm, dim3(1), dim3(1024), 0, (const double *)x, s.W, scal, (double *)nullptr);
}

// steps `step` and `step + 1`; lbs[0 .. 2 * step + 4): every lower bound so far, ||du x|| and ||du^T y|| per step
template <typename T> static int power_two_steps(NormScratch &s, const T *un, const T *uo, int step, double *lbs)
{
    const int W = s.W, H = s.H;
    double *x = s.pw_x.as<double>(), *y = s.pw_y.as<double>(), *scal = s.pw_scal.as<double>();
    for (int st = step; st < step + 2; st++) {
        TF_TRY(launch("hs_power", k_pw_rows<T>, dim3(H), dim3(256), 0, un, uo, W, (const double *)x, (const double *)scal, y));
        TF_TRY(launch("hs_power", k_norm, dim3(1), dim3(1024), 0, (const double *)y, H, scal + 1, scal + 2 + 2 * st));
        TF_TRY(launch("hs_power", k_pw_cols<T>, dim3(cdiv(W, 256), PW_CHUNKS), dim3(256), 0, un, uo, W, H, (const double *)y,
                      (const double *)(scal + 1), s.pw_xpart.as<double>()));
        TF_TRY(launch("hs_power", k_pw_combine, dim3(cdiv(W, 256)), dim3(256), 0, (const double *)s.pw_xpart.p, W, x));
        TF_TRY(launch("hs_power", k_norm, dim3(1), dim3(1024), 0, (const double *)x, W, scal, scal + 3 + 2 * st));
    }
    TF_HIP(hipMemcpyAsync(lbs, scal + 2, (size_t)(2 * step + 4) * sizeof(double), hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

// Gram certificate: the walk over G, G^2, G^4, each in one of the two scratch buffers
struct GramWalk {
    int p = 0;
    double *src = nullptr, *dst = nullptr;
};

static bool gram_usable(double F) { return F > 0 && std::isfinite(F); }

// A = du / F, then G = A A^T
template <typename T> static int gram_start(NormScratch &s, const T *un, const T *uo, double F, GramWalk &g)
{
    const int W = s.W, H = s.H, p = W < H ? W : H, m = W < H ? H : W;
    if (s.gram_a.bytes < (size_t)p * m * sizeof(double))
        TF_TRY(s.gram_a.alloc((size_t)p * m * sizeof(double)));
    if (s.gram_g.bytes < (size_t)p * p * sizeof(double))
        TF_TRY(s.gram_g.alloc((size_t)p * p * sizeof(double)));
    double *A = s.gram_a.as<double>(), *G = s.gram_g.as<double>();
    TF_TRY(launch("hs_gram_build", k_gram_build<T>, dim3(cdiv((size_t)W * H, 256)), dim3(256), 0, un, uo, W, H, 1.0 / F, A));
    TF_TRY(launch("hs_gram_syrk", k_syrk, dim3(cdiv(p, 64), cdiv(p, 64)), dim3(256), 0, (const double *)A, p, m, G));
    g.p = p, g.src = G, g.dst = A;
    return TF_OK;
}

// the bound of k = 1, 2, 4 in turn: sigma <= F ||G^k||_F^(1 / (2k))
static int gram_bound(NormScratch &s, GramWalk &g, int k, double F, double *bound)
{
    if (k > 1) { // G^k = G^(k/2) (G^(k/2))^T: the powers are symmetric
        TF_TRY(launch("hs_gram_syrk", k_syrk, dim3(cdiv(g.p, 64), cdiv(g.p, 64)), dim3(256), 0, (const double *)g.src, g.p, g.p,
                      g.dst));
        std::swap(g.src, g.dst);
    }
    double fro;
    TF_TRY(frobenius(s, g.src, (size_t)g.p * g.p, &fro));
    *bound = F * std::pow(fro, 1.0 / (2 * k));
    return TF_OK;
}

template <typename T>
static int decide_device_t(NormScratch &s, const T *un, const T *uo, double delta, double F, int *decision, int *stage)
{
    const double hi = delta * (1 + GUARD), lo = delta * (1 - GUARD);
    // 2. power iteration
    double lbs[2 * POWER_STEPS];
    TF_TRY(power_start(s));
    for (int step = 0; step < POWER_STEPS; step += 2) {
        TF_TRY(power_two_steps(s, un, uo, step, lbs));
        for (int k = 0; k < 2 * step + 4; k++)
            if (lbs[k] >= hi) {
                *decision = NOT_CONVERGED, *stage = ST_POWER;
                return TF_OK;
            }
    }
    // 3. Gram certificate
    if (gram_usable(F)) {
        GramWalk g;
        TF_TRY(gram_start(s, un, uo, F, g));
        for (int k = 1; k <= 4; k *= 2) {
            double bound;
            TF_TRY(gram_bound(s, g, k, F, &bound));
            if (bound < lo) {
                *decision = CONVERGED, *stage = ST_GRAM;
                return TF_OK;
            }
        }
    }
    *decision = UNDECIDED, *stage = ST_HOST;
    return TF_OK;
}

int decide_device(NormScratch &s, const void *u_new, const void *u_old, bool f64, double delta, double F, int *decision, int *stage)
{
    if (f64)
        return decide_device_t(s, (const double *)u_new, (const double *)u_old, delta, F, decision, stage);
    return decide_device_t(s, (const float *)u_new, (const float *)u_old, delta, F, decision, stage);
}

template <typename T> static int device_values_t(NormScratch &s, const T *un, const T *uo, double F, StageValues *v)
{
    TF_TRY(power_start(s));
    for (int step = 0; step < POWER_STEPS; step += 2)
        TF_TRY(power_two_steps(s, un, uo, step, v->power));
    v->gram[0] = v->gram[1] = v->gram[2] = std::numeric_limits<double>::quiet_NaN();
    if (gram_usable(F)) {
        GramWalk g;
        TF_TRY(gram_start(s, un, uo, F, g));
        for (int k = 1, i = 0; k <= 4; k *= 2, i++)
            TF_TRY(gram_bound(s, g, k, F, &v->gram[i]));
    }
    return TF_OK;
}

int device_values(NormScratch &s, const void *u_new, const void *u_old, bool f64, double F, StageValues *v)
{
    if (f64)
        return device_values_t(s, (const double *)u_new, (const double *)u_old, F, v);
    return device_values_t(s, (const float *)u_new, (const float *)u_old, F, v);
}

} // namespace hs
} // namespace tf

using namespace tf;
using namespace tf::hs;

// A host field pair on the device and its cheap bounds, by the stage entry's partials kernel and the product's reduction
struct StagedField {
    NormScratch s;
    DevBuf un, uo;
    Bounds b;
};

static int stage_field(StagedField &f, const void *u_new, const void *u_old, int w, int h, bool f64)
{
    TF_TRY(ensure_init());
    TF_TRY(f.s.init(w, h));
    const size_t bytes = (size_t)w * h * (f64 ? 8 : 4);
    TF_TRY(f.un.alloc(bytes));
    TF_TRY(f.uo.alloc(bytes));
    TF_HIP(hipMemcpyAsync(f.un.p, u_new, bytes, hipMemcpyHostToDevice, stream()));
    if (u_old)
        TF_HIP(hipMemcpyAsync(f.uo.p, u_old, bytes, hipMemcpyHostToDevice, stream()));
    else
        TF_HIP(hipMemsetAsync(f.uo.p, 0, bytes, stream()));   // du = u_new - 0 = u_new
    TF_TRY(launch_delta_partials(f.un.p, f.uo.p, f64, w, h, f.s.partials.as<double>()));
    PairList pl;
    pl.n = 1;
    pl.p[0] = PairDesc{0, 0};
    TF_TRY(launch_bounds_reduce(f.s.partials.as<double>(), 0, pl, w, h, f.s.blocks.as<double>()));
    TF_HIP(hipMemcpyAsync(f.s.host_blocks.data(), f.s.blocks.p, f.s.host_blocks.size() * sizeof(double), hipMemcpyDeviceToHost,
                          stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    f.b = bounds_of(f.s.host_blocks.data(), w, h);
    return TF_OK;
}

TF_API int tf_hs_stage_norm_test(const void *field, int w, int h, int is_f64, double delta, int *decision, int *stage)
{
    TF_REQUIRE(field && decision && stage, "tf_hs_stage_norm_test: null pointer");
    TF_REQUIRE(w >= 1 && h >= 1 && (long long)w * h < (1ll << 31), "tf_hs_stage_norm_test: bad size %dx%d", w, h);
    StagedField f;
    TF_TRY(stage_field(f, field, nullptr, w, h, is_f64 != 0));
    *decision = decide_bounds(f.b, delta);
    *stage = ST_BOUNDS;
    if (*decision == UNDECIDED && f.b.device_stages())
        TF_TRY(decide_device(f.s, f.un.p, f.uo.p, is_f64 != 0, delta, f.b.F, decision, stage));
    if (*decision == UNDECIDED)
        *stage = ST_HOST;
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

TF_API int tf_hs_stage_norm_values(const void *u_new, const void *u_old, int w, int h, int is_f64, double *out)
{
    TF_REQUIRE(u_new && out, "tf_hs_stage_norm_values: null pointer");
    TF_REQUIRE(w >= 1 && h >= 1 && (long long)w * h < (1ll << 31), "tf_hs_stage_norm_values: bad size %dx%d", w, h);
    StagedField f;
    TF_TRY(stage_field(f, u_new, u_old, w, h, is_f64 != 0));
    out[0] = f.b.F, out[1] = f.b.U, out[2] = f.b.L;
    StageValues v;
    for (double &x : v.power)
        x = std::numeric_limits<double>::quiet_NaN();
    for (double &x : v.gram)
        x = std::numeric_limits<double>::quiet_NaN();
    if (f.b.device_stages())
        TF_TRY(device_values(f.s, f.un.p, f.uo.p, is_f64 != 0, f.b.F, &v));
    for (int k = 0; k < 2 * POWER_STEPS; k++)
        out[3 + k] = v.power[k];
    for (int k = 0; k < 3; k++)
        out[3 + 2 * POWER_STEPS + k] = v.gram[k];
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}
