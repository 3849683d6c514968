// Per-value rules of the flow-array kernels, written once for flowops.hip (one array in, one array out) and
// flowseam.hip (the same steps fused for flows that stay on the device):
//   the merge of n operands     transflow/pipeline.py:149-158, transflow/utils.py:359-381
//   render1d's pixel            transflow/output/render.py:9-27
#pragma once
#include "common.h"

namespace tf {

// N values that go through a rule side by side (the loops over N unroll: the values stay in registers)
template <int N> struct Vals {
    float v[N];
};

// Pipeline.FLOW_MERGING_FUNCTIONS: float32, operands combined left to right; load(i) gives operand i's values.
// numpy.sum starts from the identity of add and Python's sum() from 0, so both sums start from +0.0: operands that
// are all -0.0 sum to +0.0
template <int N, typename Load> __device__ __forceinline__ Vals<N> merge_rule(int kind, int n, Load load)
{
    Vals<N> r = load(0);
    switch (kind) {
    case TF_MERGE_FIRST:
        break;
    case TF_MERGE_SUM:
    case TF_MERGE_AVERAGE:
#pragma unroll
        for (int k = 0; k < N; k++)
            r.v[k] = 0.f + r.v[k];
        for (int i = 1; i < n; i++) {
            const Vals<N> x = load(i);
#pragma unroll
            for (int k = 0; k < N; k++)
                r.v[k] = r.v[k] + x.v[k];
        }
        if (kind == TF_MERGE_AVERAGE) {
#pragma unroll
            for (int k = 0; k < N; k++)
                r.v[k] = r.v[k] / (float)n;
        }
        break;
    case TF_MERGE_DIFFERENCE: { // flows[0] - sum(flows[1:])
        Vals<N> s;
#pragma unroll
        for (int k = 0; k < N; k++)
            s.v[k] = 0.f;
        for (int i = 1; i < n; i++) {
            const Vals<N> x = load(i);
#pragma unroll
            for (int k = 0; k < N; k++)
                s.v[k] = s.v[k] + x.v[k];
        }
#pragma unroll
        for (int k = 0; k < N; k++)
            r.v[k] = r.v[k] - s.v[k];
        break;
    }
    case TF_MERGE_PRODUCT:
        for (int i = 1; i < n; i++) {
            const Vals<N> x = load(i);
#pragma unroll
            for (int k = 0; k < N; k++)
                r.v[k] = r.v[k] * x.v[k];
        }
        break;
    case TF_MERGE_MASKBIN: // utils.py:367-373: |x| > 0.2 (float32) -> 1, else 0
        for (int i = 1; i < n; i++) {
            const Vals<N> x = load(i);
#pragma unroll
            for (int k = 0; k < N; k++)
                r.v[k] = r.v[k] * (fabsf(x.v[k]) > 0.2f ? 1.f : 0.f);
        }
        break;
    case TF_MERGE_MASKLIN:
        for (int i = 1; i < n; i++) {
            const Vals<N> x = load(i);
#pragma unroll
            for (int k = 0; k < N; k++)
                r.v[k] = r.v[k] * fabsf(x.v[k]);
        }
        break;
    case TF_MERGE_ABSMAX: { // utils.py:376-381: numpy.argmax keeps the first maximum; a NaN is a maximum
        const Vals<N> x = load(1);
#pragma unroll
        for (int k = 0; k < N; k++) {
            const float a0 = fabsf(r.v[k]), a1 = fabsf(x.v[k]);
            if (a1 > a0 || (a1 != a1 && a0 == a0))
                r.v[k] = x.v[k];
        }
        break;
    }
    }
    return r;
}

struct Colors {
    float c[4][3];
};

inline Colors make_colors(const float *rgb, int n)
{
    Colors c = {};
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++)
            c.c[i][k] = rgb[i * 3 + k];
    return c;
}

__device__ __forceinline__ float clip01(float v) { return clip_nan(v, 0.f, 1.f); }
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)(int)clip_nan(v, 0.f, 255.f); }

// output/render.py:19-27 for one value: the pixel's three bytes
__device__ __forceinline__ void render1d_rule(float a, float scale, const Colors &col, int binary, uint8_t *px)
{
    const float sa = scale * a;
    float ka, kb;
    if (binary) {
        kb = clip01(rintf(sa));
        ka = 1.f - kb;
    } else {
        ka = clip01(1.f - sa);
        kb = clip01(sa);
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
        px[c] = to_u8(ka * col.c[0][c] + kb * col.c[1][c]);
}

} // namespace tf
