// Horn-Schunck optical flow (transflow/flow/methods/horn_schunck.py), bit for bit: the prepare kernel (blur and
// derivatives), the iteration kernel of both dtype chains, and the tf_hs_* entry points.  DESIGN.md section 10.
//
// Rounding, statement by statement (compiled with -ffp-contract=off, so no multiply-add is fused):
//  - cv2.GaussianBlur(float32, (5, 5), 0) is the fixed kernel [1, 4, 6, 4, 1] / 16 with BORDER_REFLECT_101.  On uint8
//    values every partial sum is a multiple of 1/256 below 256, exact in float32: computed here as an integer sum / 256.
//  - scipy.ndimage.convolve (mode "reflect") sums the nonzero taps of the flipped kernel in C order, from 0.0, in
//    float64, and casts to the input's dtype.  The 2x2 kernels read (i..i+1, j..j+1), the 3x3 average is centred;
//    "reflect" repeats the edge sample (index -1 -> 0, n -> n - 1).  ex, ey, et are exact in any order.
//  - den = (float(alpha ** 2) + ex * ex) + ey * ey in float32 in both chains.
//  - float32 chain: u_avg = float(sum); c = ((ex * u_avg + ey * v_avg) + et) / den; u = u_avg - ex * c, all float32.
//  - float64 chain: the same with u_avg, c, u, v in float64 and ex, ey, et, den widened.
#include "hs_common.h"

namespace tf {
namespace hs {

__device__ __forceinline__ int refl101(int i, int n)
{
    if (n == 1)
        return 0;
    while (i < 0 || i >= n) {
        if (i < 0)
            i = -i;
        if (i >= n)
            i = 2 * n - 2 - i;
    }
    return i;
}

struct SlotPairs {
    int prev[MAX_PAIRS], next[MAX_PAIRS];
};

// ---- prepare: two uint8 frames -> {ex, ey, et, den} -------------------------------------------------------------
constexpr int PX = 32, PY = 8;   // outputs per block; the blurred tile is (PY + 1) x (PX + 1)

__global__ __launch_bounds__(256) void k_hs_prepare(const uint8_t *__restrict__ frames, SlotPairs sp, int W, int H,
                                                    float alpha_sq, float4 *__restrict__ deriv)
{
    __shared__ int hsum[2][PY + 5][PX + 1];     // horizontal 5-tap sums of the raw rows the tile needs
    __shared__ float bl[2][PY + 1][PX + 1];     // blurred frames
    const int z = blockIdx.z;
    const size_t npx = (size_t)W * H;
    const uint8_t *img[2] = {frames + (size_t)sp.prev[z] * npx, frames + (size_t)sp.next[z] * npx};
    const int x0 = blockIdx.x * PX, y0 = blockIdx.y * PY, t = threadIdx.x;
    // raw row rr of the tile is image row refl101(y0 - 2 + rr); tile column m is image column min(x0 + m, W - 1)
    for (int e = t; e < 2 * (PY + 5) * (PX + 1); e += 256) {
        const int f = e / ((PY + 5) * (PX + 1)), rem = e % ((PY + 5) * (PX + 1));
        const int rr = rem / (PX + 1), m = rem % (PX + 1);
        const uint8_t *row = img[f] + (size_t)refl101(y0 - 2 + rr, H) * W;
        const int cm = min(x0 + m, W - 1);
        hsum[f][rr][m] = row[refl101(cm - 2, W)] + 4 * row[refl101(cm - 1, W)] + 6 * row[cm] + 4 * row[refl101(cm + 1, W)] +
                         row[refl101(cm + 2, W)];
    }
    __syncthreads();
    // blurred row k is image row min(y0 + k, H - 1): a row past the bottom repeats the last (scipy "reflect" of the
    // 2x2 stencils), whose raw rows start at tile row H - 1 - y0
    for (int e = t; e < 2 * (PY + 1) * (PX + 1); e += 256) {
        const int f = e / ((PY + 1) * (PX + 1)), rem = e % ((PY + 1) * (PX + 1));
        const int k = min(rem / (PX + 1), H - 1 - y0), m = rem % (PX + 1);
        const int s = hsum[f][k][m] + 4 * hsum[f][k + 1][m] + 6 * hsum[f][k + 2][m] + 4 * hsum[f][k + 3][m] + hsum[f][k + 4][m];
        bl[f][rem / (PX + 1)][m] = (float)s / 256.0f;
    }
    __syncthreads();
    const int tx = t % PX, ty = t / PX, x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H)
        return;
    float cx[2], cy[2], ct[2];
    for (int f = 0; f < 2; f++) {
        const double a00 = bl[f][ty][tx], a01 = bl[f][ty][tx + 1], a10 = bl[f][ty + 1][tx], a11 = bl[f][ty + 1][tx + 1];
        // the flipped kernels' nonzero taps in C order
        cx[f] = (float)((((0.0 + a00 * -0.25) + a01 * 0.25) + a10 * -0.25) + a11 * 0.25);
        cy[f] = (float)((((0.0 + a00 * -0.25) + a01 * -0.25) + a10 * 0.25) + a11 * 0.25);
        ct[f] = (float)((((0.0 + a00 * 0.25) + a01 * 0.25) + a10 * 0.25) + a11 * 0.25);
    }
    const float ex = cx[0] + cx[1], ey = cy[0] + cy[1], et = ct[1] - ct[0];
    const float den = (alpha_sq + ex * ex) + ey * ey;
    deriv[(size_t)z * npx + (size_t)y * W + x] = make_float4(ex, ey, et, den);
}

// ---- the float32 chain's start: u = float32(decay) * flow[..., 0] ----------------------------------------------
__global__ void k_hs_init_f32(const float2 *__restrict__ flow, float decay, float *__restrict__ u, float *__restrict__ v,
                              size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const float2 f = flow[i];
    u[i] = decay * f.x;
    v[i] = decay * f.y;
}

struct IterArgs {
    const float4 *deriv;
    char *uv;                 // tf_hs::uv
    size_t plane_bytes;
    double *partials;
    size_t partial_stride;    // doubles per pair
    int W, H;
};

template <typename T> __device__ __forceinline__ T *plane_of(const IterArgs &a, int pair, int buf, int comp)
{
    return (T *)(a.uv + (((size_t)pair * 2 + buf) * 2 + comp) * a.plane_bytes);
}

// scipy.ndimage.convolve(u, [[1,2,1],[2,0,2],[1,2,1]] / 12): the eight taps in C order, float64, from 0.0
template <typename T> __device__ __forceinline__ T avg3(const T (&m)[3][3])
{
    constexpr double w1 = 1.0 / 12.0, w2 = 2.0 / 12.0;
    double s = 0.0;
    s = s + (double)m[0][0] * w1;
    s = s + (double)m[0][1] * w2;
    s = s + (double)m[0][2] * w1;
    s = s + (double)m[1][0] * w2;
    s = s + (double)m[1][2] * w2;
    s = s + (double)m[2][0] * w1;
    s = s + (double)m[2][1] * w2;
    s = s + (double)m[2][2] * w1;
    return (T)s;
}

// One iteration of every listed pair: a thread per column of a 256-column block walks down a strip of IT_ROWS rows with
// the 3x3 windows of u and v in registers (the side columns come from the neighbouring threads' lines, in cache).  Reads
// {ex, ey, et, den}, u, v; writes the new u, v into the pair's other buffer.  BOUNDS: also the strip's column sums and
// the block's row sums of du^2 and |du| (du = u_new - u_old in the chain's dtype), deterministic (fixed trees, no atomics).
template <typename T, bool BOUNDS>
__global__ __launch_bounds__(IT_BX) void k_hs_iterate(IterArgs a, PairList pl)
{
    const PairDesc pd = pl.p[blockIdx.z];
    const int W = a.W, H = a.H;
    const T *u = plane_of<T>(a, pd.pair, pd.cur, 0), *v = plane_of<T>(a, pd.pair, pd.cur, 1);
    T *un = plane_of<T>(a, pd.pair, pd.cur ^ 1, 0), *vn = plane_of<T>(a, pd.pair, pd.cur ^ 1, 1);
    const float4 *d = a.deriv + (size_t)pd.pair * W * H;
    const int c0 = blockIdx.x * IT_BX + threadIdx.x;
    const bool valid = c0 < W;
    const int c = valid ? c0 : W - 1;
    const int cl = c > 0 ? c - 1 : 0, cr = c + 1 < W ? c + 1 : W - 1;
    const int r0 = blockIdx.y * IT_ROWS, r1 = min(r0 + IT_ROWS, H);
    T mu[3][3], mv[3][3];
    {
        const int rm = r0 > 0 ? r0 - 1 : 0;
        const T *pu = u + (size_t)rm * W, *pv = v + (size_t)rm * W;
        mu[0][0] = pu[cl], mu[0][1] = pu[c], mu[0][2] = pu[cr];
        mv[0][0] = pv[cl], mv[0][1] = pv[c], mv[0][2] = pv[cr];
        pu = u + (size_t)r0 * W, pv = v + (size_t)r0 * W;
        mu[1][0] = pu[cl], mu[1][1] = pu[c], mu[1][2] = pu[cr];
        mv[1][0] = pv[cl], mv[1][1] = pv[c], mv[1][2] = pv[cr];
    }
    [[maybe_unused]] double csq = 0.0, cab = 0.0;
    __shared__ double rowred[BOUNDS ? IT_ROWS : 1][4][2];
    for (int r = r0; r < r1; r++) {
        const int rp = r + 1 < H ? r + 1 : H - 1;
        const T *pu = u + (size_t)rp * W, *pv = v + (size_t)rp * W;
        mu[2][0] = pu[cl], mu[2][1] = pu[c], mu[2][2] = pu[cr];
        mv[2][0] = pv[cl], mv[2][1] = pv[c], mv[2][2] = pv[cr];
        const float4 q = d[(size_t)r * W + c];
        const T ua = avg3(mu), va = avg3(mv);
        const T ex = (T)q.x, ey = (T)q.y, et = (T)q.z, den = (T)q.w;
        const T cc = ((ex * ua + ey * va) + et) / den;
        const T nu = ua - ex * cc, nv = va - ey * cc;
        if (valid) {
            un[(size_t)r * W + c] = nu;
            vn[(size_t)r * W + c] = nv;
        }
        if constexpr (BOUNDS) {
            const T du = nu - mu[1][1];
            const double dd = valid ? (double)du : 0.0;
            const double sq = dd * dd, ab = fabs(dd);
            csq = csq + sq;
            cab = cab + ab;
            const double wsq = wave_sum(sq), wab = wave_sum(ab);
            if ((threadIdx.x & 63) == 0) {
                rowred[r - r0][threadIdx.x >> 6][0] = wsq;
                rowred[r - r0][threadIdx.x >> 6][1] = wab;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            mu[0][k] = mu[1][k], mu[1][k] = mu[2][k];
            mv[0][k] = mv[1][k], mv[1][k] = mv[2][k];
        }
    }
    if constexpr (BOUNDS)
        strip_store(a.partials + (size_t)pd.pair * a.partial_stride, W, H, valid ? c0 : -1, blockIdx.y, blockIdx.x, r0,
                    r1 - r0, csq, cab, rowred);
}

// stack([u, v], -1).astype(float32)
template <typename T> __global__ void k_hs_output(const T *__restrict__ u, const T *__restrict__ v, float2 *__restrict__ flow, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        flow[i] = make_float2((float)u[i], (float)v[i]);
}

} // namespace hs
} // namespace tf

using namespace tf;
using namespace tf::hs;

TF_API int tf_hs_create(tf_hs **out, int width, int height, int frame_slots, int max_pairs)
{
    TF_REQUIRE(out, "tf_hs_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(width >= 1 && height >= 1 && (long long)width * height < (1ll << 31), "tf_hs_create: bad size %dx%d", width, height);
    TF_REQUIRE(frame_slots >= 2, "tf_hs_create: frame_slots %d < 2", frame_slots);
    TF_REQUIRE(max_pairs >= 1 && max_pairs <= MAX_PAIRS, "tf_hs_create: max_pairs %d not in [1, %d]", max_pairs, MAX_PAIRS);
    TF_TRY(ensure_init());
    auto hs = make_handle<tf_hs>();
    TF_REQUIRE(hs, "tf_hs_create: out of memory");
    hs->W = width, hs->H = height, hs->slots = frame_slots, hs->max_pairs = max_pairs;
    const size_t npx = (size_t)width * height;
    TF_TRY(hs->frames.alloc((size_t)frame_slots * npx));
    TF_TRY(hs->deriv.alloc((size_t)max_pairs * npx * sizeof(float4)));
    TF_TRY(hs->uv.alloc((size_t)max_pairs * 4 * hs->plane_bytes()));
    TF_TRY(hs->init_flow.alloc((size_t)max_pairs * npx * 2 * sizeof(float)));
    TF_TRY(hs->flow.alloc((size_t)max_pairs * npx * 2 * sizeof(float)));
    TF_TRY(hs->partials.alloc((size_t)max_pairs * partial_doubles(width, height) * sizeof(double)));
    TF_TRY(hs->blocks.alloc((size_t)max_pairs * n_bound_blocks(width, height) * 4 * sizeof(double)));
    TF_TRY(hs->norm.init(width, height));
    hs->host_blocks.resize((size_t)max_pairs * n_bound_blocks(width, height) * 4);
    hs->has_init.assign(max_pairs, 0);
    hs->init_dev.assign(max_pairs, nullptr);
    hs->state.assign(max_pairs, tf_hs::DONE);
    hs->iter.assign(max_pairs, 0);
    hs->cur.assign(max_pairs, 0);
    hs->f64.assign(max_pairs, 1);
    hs->stats.assign(max_pairs, {0, 0, 0, 0, 0});
    *out = hs.release();
    return TF_OK;
}

TF_API void tf_hs_destroy(tf_hs *hs)
{
    if (hs)
        (void)hipStreamSynchronize(stream()); // kernels of the handle's last call may still read its buffers
    delete hs;
}

TF_API int tf_hs_set_frame(tf_hs *hs, int slot, const uint8_t *grey, ptrdiff_t stride)
{
    TF_REQUIRE(hs && grey, "tf_hs_set_frame: null pointer");
    TF_REQUIRE(slot >= 0 && slot < hs->slots, "tf_hs_set_frame: slot %d out of range (%d slots)", slot, hs->slots);
    TF_REQUIRE(stride >= hs->W, "tf_hs_set_frame: stride %td smaller than width %d", stride, hs->W);
    uint8_t *dst = hs->frames.as<uint8_t>() + (size_t)slot * hs->W * hs->H;
    TF_HIP(hipMemcpy2DAsync(dst, hs->W, grey, (size_t)stride, hs->W, hs->H, hipMemcpyHostToDevice, stream()));
    TF_HIP(hipStreamSynchronize(stream())); // the host frame is borrowed for this call only
    return TF_OK;
}

// cv.py:461-466 on the device, as tf_fb_set_frame_bgr: nearest-neighbour resize and BGR -> grey into the slot
TF_API int tf_hs_set_frame_bgr(tf_hs *hs, int slot, const uint8_t *bgr, int src_width, int src_height, ptrdiff_t stride)
{
    TF_REQUIRE(hs && bgr, "tf_hs_set_frame_bgr: null pointer");
    TF_REQUIRE(slot >= 0 && slot < hs->slots, "tf_hs_set_frame_bgr: slot %d out of range (%d slots)", slot, hs->slots);
    TF_REQUIRE(src_width >= 1 && src_height >= 1 && (long long)src_width * src_height < (1ll << 31),
               "tf_hs_set_frame_bgr: bad source size %dx%d", src_width, src_height);
    TF_REQUIRE(stride >= (ptrdiff_t)3 * src_width, "tf_hs_set_frame_bgr: stride %td smaller than a row of %d BGR pixels", stride,
               src_width);
    const size_t row = (size_t)3 * src_width, need = row * src_height;
    if (hs->bgr_stage.bytes < need)
        TF_TRY(hs->bgr_stage.alloc(need));
    uint8_t *dst = hs->frames.as<uint8_t>() + (size_t)slot * hs->W * hs->H;
    TF_HIP(hipMemcpy2DAsync(hs->bgr_stage.p, row, bgr, (size_t)stride, row, src_height, hipMemcpyHostToDevice, stream()));
    TF_TRY(tf_frame_grey_dev(hs->bgr_stage.p, src_width, src_height, dst, hs->W, hs->H));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

TF_API int tf_hs_set_initial_flow(tf_hs *hs, int pair, const float *flow)
{
    TF_REQUIRE(hs, "tf_hs_set_initial_flow: null handle");
    TF_REQUIRE(pair >= 0 && pair < hs->max_pairs, "tf_hs_set_initial_flow: pair %d out of range", pair);
    hs->init_dev[pair] = nullptr;
    if (!flow) {
        hs->has_init[pair] = 0;
        return TF_OK;
    }
    const size_t bytes = (size_t)hs->W * hs->H * 2 * sizeof(float);
    TF_HIP(hipMemcpyAsync((char *)hs->init_flow.p + (size_t)pair * bytes, flow, bytes, hipMemcpyHostToDevice, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    hs->has_init[pair] = 1;
    return TF_OK;
}

TF_API int tf_hs_set_initial_flow_dev(tf_hs *hs, int pair, const void *flow_dev)
{
    TF_REQUIRE(hs, "tf_hs_set_initial_flow_dev: null handle");
    TF_REQUIRE(pair >= 0 && pair < hs->max_pairs, "tf_hs_set_initial_flow_dev: pair %d out of range", pair);
    TF_REQUIRE((uintptr_t)flow_dev % 8 == 0, "tf_hs_set_initial_flow_dev: the flow must be 8-byte aligned");
    hs->init_dev[pair] = flow_dev; // borrowed: k_hs_init_f32 of the next call reads it, in stream order
    hs->has_init[pair] = flow_dev != nullptr;
    return TF_OK;
}

static int hs_output(tf_hs *hs)
{
    const size_t n = (size_t)hs->W * hs->H;
    for (int p = 0; p < hs->n_pairs; p++) {
        float2 *out = (float2 *)hs->flow.p + (size_t)p * n;
        const void *u = hs->plane(p, hs->cur[p], 0), *v = hs->plane(p, hs->cur[p], 1);
        if (hs->f64[p])
            TF_TRY(launch("hs_output", k_hs_output<double>, dim3(cdiv(n, 256)), dim3(256), 0, (const double *)u,
                          (const double *)v, out, n));
        else
            TF_TRY(launch("hs_output", k_hs_output<float>, dim3(cdiv(n, 256)), dim3(256), 0, (const float *)u,
                          (const float *)v, out, n));
    }
    hs->last_pairs = hs->n_pairs;
    return TF_OK;
}

static int hs_launch_iterate(tf_hs *hs, const PairList &pl, bool f64, bool bounds)
{
    if (pl.n == 0)
        return TF_OK;
    IterArgs a{hs->deriv.as<float4>(), (char *)hs->uv.p, hs->plane_bytes(), hs->partials.as<double>(),
               partial_doubles(hs->W, hs->H), hs->W, hs->H};
    const dim3 grid(n_colblocks(hs->W), n_strips(hs->H), pl.n);
    if (f64)
        return bounds ? launch("hs_iterate_f64", k_hs_iterate<double, true>, grid, dim3(IT_BX), 0, a, pl)
                      : launch("hs_iterate_f64", k_hs_iterate<double, false>, grid, dim3(IT_BX), 0, a, pl);
    return bounds ? launch("hs_iterate_f32", k_hs_iterate<float, true>, grid, dim3(IT_BX), 0, a, pl)
                  : launch("hs_iterate_f32", k_hs_iterate<float, false>, grid, dim3(IT_BX), 0, a, pl);
}

// Iterations of every running pair until each is done or waits for the host.
static int hs_run(tf_hs *hs)
{
    const int nbb = n_bound_blocks(hs->W, hs->H);
    const bool has_delta = hs->prm.has_delta != 0;
    for (;;) {
        PairList l[2];
        l[0].n = l[1].n = 0;
        for (int p = 0; p < hs->n_pairs; p++)
            if (hs->state[p] == tf_hs::RUNNING) {
                PairList &li = l[hs->f64[p]];
                li.p[li.n++] = PairDesc{p, hs->cur[p]};
            }
        if (l[0].n + l[1].n == 0)
            break;
        for (int k = 0; k < 2; k++)
            TF_TRY(hs_launch_iterate(hs, l[k], k == 1, has_delta));
        for (int k = 0; k < 2; k++)
            for (int i = 0; i < l[k].n; i++) {
                const int p = l[k].p[i].pair;
                hs->cur[p] ^= 1;
                hs->iter[p]++;
                hs->stats[p][0]++;
            }
        if (has_delta) {
            for (int k = 0; k < 2; k++)
                if (l[k].n)
                    TF_TRY(launch_bounds_reduce(hs->partials.as<double>(), partial_doubles(hs->W, hs->H), l[k], hs->W, hs->H,
                                                hs->blocks.as<double>()));
            TF_HIP(hipMemcpyAsync(hs->host_blocks.data(), hs->blocks.p, (size_t)hs->n_pairs * nbb * 4 * sizeof(double),
                                  hipMemcpyDeviceToHost, stream()));
            TF_HIP(hipStreamSynchronize(stream()));
            for (int k = 0; k < 2; k++)
                for (int i = 0; i < l[k].n; i++) {
                    const int p = l[k].p[i].pair;
                    const Bounds b = bounds_of(hs->host_blocks.data() + (size_t)p * nbb * 4, hs->W, hs->H);
                    int dec = decide_bounds(b, hs->prm.delta);
                    int stage = ST_BOUNDS;
                    if (dec == UNDECIDED && b.device_stages())
                        TF_TRY(decide_device(hs->norm, hs->plane(p, hs->cur[p], 0), hs->plane(p, hs->cur[p] ^ 1, 0), k == 1,
                                             hs->prm.delta, b.F, &dec, &stage));
                    if (dec == UNDECIDED)
                        stage = ST_HOST;
                    hs->stats[p][1 + stage]++;
                    if (dec == CONVERGED)
                        hs->state[p] = tf_hs::DONE;
                    else if (dec == UNDECIDED)
                        hs->state[p] = tf_hs::WAITING;
                }
        }
        for (int p = 0; p < hs->n_pairs; p++)
            if (hs->state[p] == tf_hs::RUNNING && hs->iter[p] >= hs->prm.max_iters)
                hs->state[p] = tf_hs::DONE;
    }
    for (int p = 0; p < hs->n_pairs; p++)
        if (hs->state[p] == tf_hs::WAITING)
            return TF_OK;
    return hs_output(hs);
}

TF_API int tf_hs_calc_slots(tf_hs *hs, const tf_hs_params *params, int n_pairs, const int *prev_slots, const int *next_slots)
{
    TF_REQUIRE(hs && params && prev_slots && next_slots, "tf_hs_calc_slots: null pointer");
    TF_REQUIRE(n_pairs >= 1 && n_pairs <= hs->max_pairs, "tf_hs_calc_slots: %d pairs (handle takes 1..%d)", n_pairs, hs->max_pairs);
    SlotPairs sp;
    for (int i = 0; i < n_pairs; i++) {
        TF_REQUIRE(prev_slots[i] >= 0 && prev_slots[i] < hs->slots && next_slots[i] >= 0 && next_slots[i] < hs->slots,
                   "tf_hs_calc_slots: pair %d: slots (%d, %d) out of range (%d slots)", i, prev_slots[i], next_slots[i], hs->slots);
        sp.prev[i] = prev_slots[i];
        sp.next[i] = next_slots[i];
    }
    hs->prm = *params;
    hs->n_pairs = n_pairs;
    hs->last_pairs = 0;
    const size_t n = (size_t)hs->W * hs->H;
    for (int p = 0; p < n_pairs; p++) {
        hs->state[p] = params->max_iters > 0 ? tf_hs::RUNNING : tf_hs::DONE;
        hs->iter[p] = 0;
        hs->cur[p] = 0;
        hs->f64[p] = !hs->has_init[p];
        hs->stats[p] = {0, 0, 0, 0, 0};
        if (hs->f64[p]) { // numpy.zeros: +0.0
            TF_HIP(hipMemsetAsync(hs->plane(p, 0, 0), 0, hs->plane_bytes(), stream()));
            TF_HIP(hipMemsetAsync(hs->plane(p, 0, 1), 0, hs->plane_bytes(), stream()));
        } else {
            const float2 *init = hs->init_dev[p] ? (const float2 *)hs->init_dev[p] : (const float2 *)hs->init_flow.p + (size_t)p * n;
            TF_TRY(launch("hs_init", k_hs_init_f32, dim3(cdiv(n, 256)), dim3(256), 0, init, (float)params->decay, (float *)hs->plane(p, 0, 0),
                          (float *)hs->plane(p, 0, 1), n));
        }
        hs->has_init[p] = 0; // an initial flow serves one call
        hs->init_dev[p] = nullptr;
    }
    TF_TRY(launch("hs_prepare", k_hs_prepare, dim3(cdiv(hs->W, PX), cdiv(hs->H, PY), n_pairs), dim3(256), 0,
                  hs->frames.as<const uint8_t>(), sp, hs->W, hs->H, (float)params->alpha_sq, hs->deriv.as<float4>()));
    return hs_run(hs);
}

TF_API int tf_hs_waiting(tf_hs *hs, int *pairs_out, int *n_waiting)
{
    TF_REQUIRE(hs && n_waiting, "tf_hs_waiting: null pointer");
    int n = 0;
    for (int p = 0; p < hs->n_pairs; p++)
        if (hs->state[p] == tf_hs::WAITING) {
            if (pairs_out)
                pairs_out[n] = p;
            n++;
        }
    *n_waiting = n;
    return TF_OK;
}

TF_API int tf_hs_delta_download(tf_hs *hs, int pair, void *out, int *is_f64)
{
    TF_REQUIRE(hs && out && is_f64, "tf_hs_delta_download: null pointer");
    TF_REQUIRE(pair >= 0 && pair < hs->n_pairs && hs->state[pair] == tf_hs::WAITING, "tf_hs_delta_download: pair %d is not waiting", pair);
    const size_t n = (size_t)hs->W * hs->H;
    const bool f64 = hs->f64[pair] != 0;
    // (the Gram buffer is at least W * H doubles once allocated; the partials of the stage entry are not in use here)
    if (hs->norm.gram_a.bytes < n * 8)
        TF_TRY(hs->norm.gram_a.alloc(n * 8));
    TF_TRY(launch_delta(hs->plane(pair, hs->cur[pair], 0), hs->plane(pair, hs->cur[pair] ^ 1, 0), f64, n, hs->norm.gram_a.p));
    TF_HIP(hipMemcpyAsync(out, hs->norm.gram_a.p, n * (f64 ? 8 : 4), hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    *is_f64 = f64;
    return TF_OK;
}

TF_API int tf_hs_resolve(tf_hs *hs, int pair, int converged)
{
    TF_REQUIRE(hs, "tf_hs_resolve: null handle");
    TF_REQUIRE(pair >= 0 && pair < hs->n_pairs && hs->state[pair] == tf_hs::WAITING, "tf_hs_resolve: pair %d is not waiting", pair);
    hs->state[pair] = converged || hs->iter[pair] >= hs->prm.max_iters ? tf_hs::DONE : tf_hs::RUNNING;
    return TF_OK;
}

TF_API int tf_hs_resume(tf_hs *hs)
{
    TF_REQUIRE(hs, "tf_hs_resume: null handle");
    for (int p = 0; p < hs->n_pairs; p++)
        TF_REQUIRE(hs->state[p] != tf_hs::WAITING, "tf_hs_resume: pair %d still waits for tf_hs_resolve", p);
    return hs_run(hs);
}

TF_API int tf_hs_get_flow(tf_hs *hs, int pair, float *flow_out)
{
    TF_REQUIRE(hs && flow_out, "tf_hs_get_flow: null pointer");
    TF_REQUIRE(pair >= 0 && pair < hs->last_pairs, "tf_hs_get_flow: pair %d was not computed by the last call", pair);
    const size_t bytes = (size_t)hs->W * hs->H * 2 * sizeof(float);
    TF_HIP(hipMemcpyAsync(flow_out, (char *)hs->flow.p + (size_t)pair * bytes, bytes, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

TF_API int tf_hs_flow_ptr(tf_hs *hs, int pair, void **dev)
{
    TF_REQUIRE(hs && dev, "tf_hs_flow_ptr: null pointer");
    TF_REQUIRE(pair >= 0 && pair < hs->last_pairs, "tf_hs_flow_ptr: pair %d was not computed by the last call", pair);
    *dev = (char *)hs->flow.p + (size_t)pair * hs->W * hs->H * 2 * sizeof(float);
    return TF_OK;
}

TF_API int tf_hs_stats(tf_hs *hs, int pair, int *stats)
{
    TF_REQUIRE(hs && stats, "tf_hs_stats: null pointer");
    TF_REQUIRE(pair >= 0 && pair < hs->n_pairs, "tf_hs_stats: pair %d out of range", pair);
    for (int k = 0; k < 5; k++)
        stats[k] = hs->stats[pair][k];
    return TF_OK;
}

TF_API int tf_hs_stage_last_bounds(tf_hs *hs, int pair, double *out)
{
    TF_REQUIRE(hs && out, "tf_hs_stage_last_bounds: null pointer");
    TF_REQUIRE(pair >= 0 && pair < hs->n_pairs, "tf_hs_stage_last_bounds: pair %d out of range", pair);
    const std::array<int, 5> &st = hs->stats[pair];
    TF_REQUIRE(st[1] + st[2] + st[3] + st[4] > 0, "tf_hs_stage_last_bounds: pair %d had no convergence check in the last call", pair);
    const Bounds b = bounds_of(hs->host_blocks.data() + (size_t)pair * n_bound_blocks(hs->W, hs->H) * 4, hs->W, hs->H);
    out[0] = b.F, out[1] = b.U, out[2] = b.L;
    return TF_OK;
}

TF_API int tf_hs_stage_derivatives(tf_hs *hs, const uint8_t *prev, const uint8_t *next, double alpha_sq, float *out)
{
    TF_REQUIRE(hs && prev && next && out, "tf_hs_stage_derivatives: null pointer");
    TF_TRY(tf_hs_set_frame(hs, 0, prev, hs->W));
    TF_TRY(tf_hs_set_frame(hs, 1, next, hs->W));
    SlotPairs sp;
    sp.prev[0] = 0, sp.next[0] = 1;
    TF_TRY(launch("hs_prepare", k_hs_prepare, dim3(cdiv(hs->W, PX), cdiv(hs->H, PY), 1), dim3(256), 0,
                  hs->frames.as<const uint8_t>(), sp, hs->W, hs->H, (float)alpha_sq, hs->deriv.as<float4>()));
    TF_HIP(hipMemcpyAsync(out, hs->deriv.p, (size_t)hs->W * hs->H * sizeof(float4), hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}
