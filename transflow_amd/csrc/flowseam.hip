// The steps of the reference's main loop between the flow sources and the compositor, for flows that stay in HBM:
//   merge + integer upscale in one pass   transflow/pipeline.py:502-504 (FLOW_MERGING_FUNCTIONS, utils.upscale_array)
//   the flow-magnitude view               transflow/pipeline.py:515-516 (sqrt(sum(power(flow, 2), axis=2)) -> render1d)
// Both stream: every source value is read once and every output byte written once, in the widest store its address
// allows.  The per-value rules are flow_rules.h's, the ones k_flow_merge and k_render1d apply.
#include <cstring>

#include "common.h"
#include "flow_rules.h"

using namespace tf;

namespace {

constexpr int BLOCK = 256;

struct SeamArgs {
    const float2 *in[TF_MAX_MERGE];
    int n, kind;
    int W, H, wf, hf;
    FastDiv div_wf;
    uint32_t in_odd;  // bit i: flow i starts 8 bytes past a 16-byte boundary
    uint32_t out_odd; // the output does
};

// One block row of the grid per source row, one lane per PAIR of adjacent output pixels (2p, 2p + 1) of that row's
// hf output rows.  A lane merges the one or two source pixels under its pair once, scales them, and stores the pair
// to each of the hf rows: as 16 bytes where that row's pair sits on a 16-byte boundary, as two 8-byte stores where
// the row starts 8 bytes off one (odd W*wf: every other row; or an output address that is only 8-byte aligned).
// The width is chosen per output row, so every lane of a block takes the same branch.  P = 1: wf is even, both
// pixels of a pair lie under one source pixel; P = 2: they may lie under two.
template <int P> __device__ __forceinline__ void seam_row(const SeamArgs &a, float2 *__restrict__ out, int y, int xo)
{
    const int Wo = a.W * a.wf;
    const bool two = xo + 1 < Wo;                      // false only for the last lane of an odd row
    const int x0 = (int)fast_div((uint32_t)xo, a.div_wf);
    const int x1 = (P == 2 && two) ? (int)fast_div((uint32_t)xo + 1, a.div_wf) : x0;
    const size_t row = (size_t)y * a.W;
    // wf == 1 and the source row of every flow on a 16-byte boundary: the pair is one 16-byte load per flow
    const bool row_odd = (y & 1) & (a.W & 1);
    const bool wide_in = P == 2 && a.wf == 1 && (row_odd ? a.in_odd == (1u << a.n) - 1 : a.in_odd == 0);
    Vals<2 * P> r;
    if (wide_in && two) {
        r = merge_rule<2 * P>(a.kind, a.n, [&](int i) {
            const float4 v = *reinterpret_cast<const float4 *>(a.in[i] + row + x0);
            Vals<2 * P> o;
            o.v[0] = v.x, o.v[1] = v.y;
            if (P == 2)
                o.v[2 * P - 2] = v.z, o.v[2 * P - 1] = v.w;
            return o;
        });
    } else {
        r = merge_rule<2 * P>(a.kind, a.n, [&](int i) {
            const float2 u = a.in[i][row + x0];
            Vals<2 * P> o;
            o.v[0] = u.x, o.v[1] = u.y;
            if (P == 2) {
                const float2 w = a.in[i][row + x1];
                o.v[2 * P - 2] = w.x, o.v[2 * P - 1] = w.y;
            }
            return o;
        });
    }
    if (a.wf != 1 || a.hf != 1) { // utils.upscale_array: after the merge, in float32
        const float fw = (float)a.wf, fh = (float)a.hf;
#pragma unroll
        for (int k = 0; k < P; k++) {
            r.v[2 * k] = r.v[2 * k] * fw;
            r.v[2 * k + 1] = r.v[2 * k + 1] * fh;
        }
    }
    const float4 pair = make_float4(r.v[0], r.v[1], r.v[2 * P - 2], r.v[2 * P - 1]);
    const uint32_t wo_odd = (uint32_t)Wo & 1;
    for (int q = 0; q < a.hf; q++) {
        const size_t yo = (size_t)y * a.hf + q;
        float2 *o = out + yo * Wo + xo;
        const bool aligned = ((a.out_odd + ((uint32_t)yo & wo_odd)) & 1) == 0; // the row's first pixel, so every even xo
        if (aligned && two) {
            *reinterpret_cast<float4 *>(o) = pair;
        } else {
            o[0] = make_float2(pair.x, pair.y);
            if (two)
                o[1] = make_float2(pair.z, pair.w);
        }
    }
}

__global__ void __launch_bounds__(BLOCK) k_flow_seam(SeamArgs a, float2 *__restrict__ out)
{
    const int Wo = a.W * a.wf;
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= ((uint32_t)Wo + 1) / 2)
        return;
    const int xo = (int)(2 * p);
    for (int y = blockIdx.y; y < a.H; y += gridDim.y) {
        if (a.wf & 1)
            seam_row<2>(a, out, y, xo);
        else
            seam_row<1>(a, out, y, xo);
    }
}

// pipeline.py:515-516: the magnitude of four vectors (32 bytes in: two 16-byte loads where the flow sits on a
// 16-byte boundary), each straight into render1d's pixel rule; 12 bytes out as three dwords.  sqrtf(x*x + y*y) is
// what numpy.sqrt(numpy.sum(numpy.power(f, 2), axis=2)) computes on float32 pairs, the form k_pp_polar uses.
__global__ void __launch_bounds__(BLOCK)
k_flow_view_mag(const float2 *__restrict__ flow, uint8_t *__restrict__ rgb, size_t N, float scale, Colors col, int binary,
                int wide_in)
{
    const size_t t4 = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * 4;
    if (t4 >= N)
        return;
    float2 f[4];
    if (t4 + 4 <= N) {
        if (wide_in) {
            const float4 u = *reinterpret_cast<const float4 *>(flow + t4), w = *reinterpret_cast<const float4 *>(flow + t4 + 2);
            f[0] = make_float2(u.x, u.y), f[1] = make_float2(u.z, u.w);
            f[2] = make_float2(w.x, w.y), f[3] = make_float2(w.z, w.w);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                f[i] = flow[t4 + i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
            f[i] = flow[min(t4 + i, N - 1)];
    }
    uint8_t px[12];
#pragma unroll
    for (int i = 0; i < 4; i++)
        render1d_rule(sqrtf(f[i].x * f[i].x + f[i].y * f[i].y), scale, col, binary, px + 3 * i);
    if (t4 + 4 <= N) {
        uint32_t *o = reinterpret_cast<uint32_t *>(rgb + t4 * 3); // t4 is a multiple of 4: 12-byte groups stay 4-aligned
#pragma unroll
        for (int d = 0; d < 3; d++)
            o[d] = px[4 * d] | (px[4 * d + 1] << 8) | (px[4 * d + 2] << 16) | ((uint32_t)px[4 * d + 3] << 24);
    } else { // the last lane: bytes, under constant indices so that px stays in registers
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (t4 + i < N) {
#pragma unroll
                for (int c = 0; c < 3; c++)
                    rgb[(t4 + i) * 3 + c] = px[3 * i + c];
            }
    }
}

} // namespace

TF_API int tf_flow_seam_dev(int kind, int n, const void *const *flows_dev, int width, int height, int wf, int hf,
                            void *out_dev)
{
    TF_REQUIRE(kind >= TF_MERGE_FIRST && kind <= TF_MERGE_ABSMAX, "tf_flow_seam: unknown kind %d", kind);
    TF_REQUIRE(n >= 1 && n <= TF_MAX_MERGE, "tf_flow_seam: %d flows (1..%d)", n, TF_MAX_MERGE);
    TF_REQUIRE(kind != TF_MERGE_ABSMAX || n == 2, "tf_flow_seam: absmax merges exactly two flows, got %d", n);
    TF_REQUIRE(width >= 0 && height >= 0 && wf >= 1 && hf >= 1, "tf_flow_seam: bad size %dx%d x(%d,%d)", width, height, wf,
               hf);
    TF_REQUIRE((long long)width * wf <= INT32_MAX && (long long)height * hf <= INT32_MAX,
               "tf_flow_seam: %dx%d x(%d,%d) is more than 2^31 - 1 pixels on a side", width, height, wf, hf);
    const bool empty = (size_t)width * height == 0;
    TF_REQUIRE(flows_dev && (out_dev || empty), "tf_flow_seam: null pointer");
    TF_REQUIRE(((uintptr_t)out_dev & 7) == 0, "tf_flow_seam: the output is not 8-byte aligned");
    SeamArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < n; i++) {
        TF_REQUIRE(flows_dev[i] || empty, "tf_flow_seam: flow %d is null", i);
        TF_REQUIRE(((uintptr_t)flows_dev[i] & 7) == 0, "tf_flow_seam: flow %d is not 8-byte aligned", i);
        a.in[i] = (const float2 *)flows_dev[i];
        a.in_odd |= (uint32_t)(((uintptr_t)flows_dev[i] >> 3) & 1) << i;
    }
    if (empty)
        return TF_OK;
    TF_TRY(ensure_init());
    a.n = n, a.kind = kind;
    a.W = width, a.H = height, a.wf = wf, a.hf = hf;
    a.div_wf = fast_div_setup((uint32_t)wf);
    a.out_odd = (uint32_t)(((uintptr_t)out_dev >> 3) & 1);
    const size_t pairs = ((size_t)width * wf + 1) / 2;
    return launch("flow_seam", k_flow_seam, dim3(cdiv(pairs, BLOCK), height < 65535 ? height : 65535), dim3(BLOCK), 0, a,
                  (float2 *)out_dev);
}

TF_API int tf_flow_view_magnitude_dev(const void *flow_dev, void *rgb_dev, size_t n_pixels, float scale,
                                      const float colors_rgb[6], int binary)
{
    TF_REQUIRE(colors_rgb && ((flow_dev && rgb_dev) || n_pixels == 0), "tf_flow_view_magnitude: null pointer");
    TF_REQUIRE(((uintptr_t)flow_dev & 7) == 0, "tf_flow_view_magnitude: the flow is not 8-byte aligned");
    TF_REQUIRE(((uintptr_t)rgb_dev & 3) == 0, "tf_flow_view_magnitude: the image is not 4-byte aligned");
    if (n_pixels == 0)
        return TF_OK;
    TF_TRY(ensure_init());
    return launch("flow_view_mag", k_flow_view_mag, dim3(cdiv((n_pixels + 3) / 4, BLOCK)), dim3(BLOCK), 0,
                  (const float2 *)flow_dev, (uint8_t *)rgb_dev, n_pixels, scale, make_colors(colors_rgb, 2), binary,
                  (int)(((uintptr_t)flow_dev & 15) == 0));
}
