// Planar YUV of an RGB frame (yuv.hip): what host and device share -- the layouts and their
// geometry, and the integer coefficients built by the section's rule.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace tf {
namespace yuv {

enum Layout { YUV444P = 0, YUV422P = 1, YUV420P = 2, NV12 = 3, N_LAYOUTS = 4 };
enum Matrix { BT601 = 0, BT709 = 1, N_MATRICES = 2 };
enum Range { TV = 0, PC = 1, N_RANGES = 2 };

constexpr int FRAC_BITS = 16; // the coefficients' fractional bits

// log2 of the chroma block's width and height in pixels
__host__ __device__ constexpr int bw_log2(int layout) { return layout == YUV444P ? 0 : 1; }
__host__ __device__ constexpr int bh_log2(int layout) { return layout == YUV420P || layout == NV12 ? 1 : 0; }

inline size_t chroma_width(int width, int layout) { return ((size_t)width + (1u << bw_log2(layout)) - 1) >> bw_log2(layout); }
inline size_t chroma_height(int height, int layout) { return ((size_t)height + (1u << bh_log2(layout)) - 1) >> bh_log2(layout); }

// Y, then U and V (planar) or the rows of U V pairs (nv12): tightly packed; 0 for what is no layout or no size
inline size_t frame_bytes(int width, int height, int layout)
{
    if (width < 1 || height < 1 || layout < 0 || layout >= N_LAYOUTS)
        return 0;
    return (size_t)width * height + 2 * chroma_width(width, layout) * chroma_height(height, layout);
}

// What the kernel is launched with.  y_add: (yo << 16) + 32768, yo = 16 (tv) or 0 (pc); the chroma's constant depends on
// the block's size only and is the kernel's own.
struct Coef {
    int32_t y[3], u[3], v[3];
    int32_t y_add;
};

// round(num / den) with halves to even; den > 0
inline int64_t rint_ratio(int64_t num, int64_t den)
{
    int64_t q = num / den, r = num % den;
    if (r < 0)
        q -= 1, r += den; // floor
    if (2 * r > den || (2 * r == den && (q & 1)))
        q += 1;
    return q;
}

// The rule of DESIGN.md section 21 in exact integer arithmetic: Kr, Kb in 1/10000; s_y = 219/255, s_c = 224/255 for tv.
// Each entry of the real row times 65536 is rounded half to even, then G takes what makes the row sum rint(s_y 65536)
// (Y) or 0 (U, V).
inline bool make_coef(int matrix, int range, Coef *c)
{
    if (matrix < 0 || matrix >= N_MATRICES || range < 0 || range >= N_RANGES)
        return false;
    const int64_t one = 10000, kr = matrix == BT601 ? 2990 : 2126, kb = matrix == BT601 ? 1140 : 722, kg = one - kr - kb;
    const int64_t sy_n = range == TV ? 219 : 1, sc_n = range == TV ? 224 : 1, s_d = range == TV ? 255 : 1;
    const int64_t unit = (int64_t)1 << FRAC_BITS;
    const int64_t yr[3] = {kr, kg, kb}, ur[3] = {-kr, -kg, one - kb}, vr[3] = {one - kr, -kg, -kb};
    for (int i = 0; i < 3; i++) {
        c->y[i] = (int32_t)rint_ratio(yr[i] * sy_n * unit, one * s_d);
        c->u[i] = (int32_t)rint_ratio(ur[i] * sc_n * unit, 2 * (one - kb) * s_d);
        c->v[i] = (int32_t)rint_ratio(vr[i] * sc_n * unit, 2 * (one - kr) * s_d);
    }
    c->y[1] += (int32_t)rint_ratio(sy_n * unit, s_d) - (c->y[0] + c->y[1] + c->y[2]);
    c->u[1] -= c->u[0] + c->u[1] + c->u[2];
    c->v[1] -= c->v[0] + c->v[1] + c->v[2];
    c->y_add = (range == TV ? 16 << FRAC_BITS : 0) + (1 << (FRAC_BITS - 1));
    return true;
}

// ---- the way back (yuvdec.hip) ----

enum Chroma { REPLICATE = 0, LINEAR = 1, N_CHROMAS = 2 };

// What the inverse kernel is launched with: R = cy y + rv v, G = cy y + gu u + gv v, B = cy y + bu u, with 16
// fractional bits; y_off: 16 (tv) or 0 (pc).
struct InvCoef {
    int32_t cy, rv, gu, gv, bu;
    int32_t y_off;
};

// The rule of DESIGN.md section 22 in exact integer arithmetic: Kr, Kb in 1/10000; s_y = 255/219, s_c = 255/224 for tv.
// Each entry is the real value times 65536, rounded half to even.
inline bool make_inv_coef(int matrix, int range, InvCoef *c)
{
    if (matrix < 0 || matrix >= N_MATRICES || range < 0 || range >= N_RANGES)
        return false;
    const int64_t one = 10000, kr = matrix == BT601 ? 2990 : 2126, kb = matrix == BT601 ? 1140 : 722, kg = one - kr - kb;
    const int64_t s_n = range == TV ? 255 : 1, sy_d = range == TV ? 219 : 1, sc_d = range == TV ? 224 : 1;
    const int64_t unit = (int64_t)1 << FRAC_BITS;
    c->cy = (int32_t)rint_ratio(s_n * unit, sy_d);
    c->rv = (int32_t)rint_ratio(2 * (one - kr) * s_n * unit, one * sc_d);
    c->gu = (int32_t)rint_ratio(-2 * (one - kb) * kb * s_n * unit, one * kg * sc_d);
    c->gv = (int32_t)rint_ratio(-2 * (one - kr) * kr * s_n * unit, one * kg * sc_d);
    c->bu = (int32_t)rint_ratio(2 * (one - kb) * s_n * unit, one * sc_d);
    c->y_off = range == TV ? 16 : 0;
    return true;
}

} // namespace yuv
} // namespace tf
