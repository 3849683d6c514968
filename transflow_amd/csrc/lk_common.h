// Lucas-Kanade (transflow/flow/methods/lukas_kanade.py -> cv2.calcOpticalFlowPyrLK): what lucaskanade.hip's kernels
// and its host code share.  The arithmetic restates OpenCV 4.x's lkpyramid.cpp (tests/lk_ref.py says which points are
// recalled rather than read); the float operations are rounded one by one (-ffp-contract=off).
#pragma once
#include "common.h"

namespace tf {
namespace lk {

constexpr int MAX_PAIRS = 64;       // pairs of one tf_lk_calc_slots call (their pointers travel as a kernel argument)
constexpr int MAX_LEVELS = TF_LK_MAX_LEVELS; // pyramid levels; min(W, H) < 2^16 gives fewer than 16 with win >= 3
constexpr int W_BITS = 14;          // the bilinear weights' fixed point
constexpr int MAX_COUNT = 30;       // criteria.maxCount
constexpr double EPS2 = 0.01 * 0.01; // criteria.epsilon squared (double)
constexpr int TRACK_BX = 256;

enum TraceCode { TR_DONE = 0, TR_LOST_PREV = 1, TR_LOST_EIG = 2, TR_LOST_NEXT = 3 };

// One level of a frame's pyramid: its size, and where its padded copy lives.  Images are uint8 and derivatives
// short2 {dx, dy}, both [h + 2P][w + 2P] with the same element offsets; `origin` is the element index of pixel (0, 0).
struct Level {
    int w, h, stride;
    long long origin;
};

struct Geometry {
    int win, P, L;                  // window, pad (= win), levels 0..L
    Level lv[MAX_LEVELS];
    long long elems;                // elements of one frame's padded pyramid
};

// The pyramid geometry of a W x H frame for a window and maxLevel: buildOpticalFlowPyramid's level count.
inline Geometry make_geometry(int W, int H, int win, int max_level)
{
    Geometry g{};
    g.win = win, g.P = win;
    int w = W, h = H, L = max_level;
    for (int l = 0; l <= max_level; l++) {
        w = (w + 1) / 2, h = (h + 1) / 2;
        if (w <= win || h <= win) {
            L = l;
            break;
        }
    }
    g.L = L;
    long long off = 0;
    w = W, h = H;
    for (int l = 0; l <= L; l++) {
        Level &v = g.lv[l];
        v.w = w, v.h = h, v.stride = w + 2 * g.P;
        v.origin = off + (long long)g.P * v.stride + g.P;
        off += (long long)v.stride * (h + 2 * g.P);
        w = (w + 1) / 2, h = (h + 1) / 2;
    }
    g.elems = off;
    return g;
}

// The frames of one call's pairs.
struct PairPtrs {
    const uint8_t *I[MAX_PAIRS];    // prev pyramid
    const uint8_t *J[MAX_PAIRS];    // next pyramid
    const short2 *D[MAX_PAIRS];     // prev derivatives
};

// cv::borderInterpolate(p, n, BORDER_REFLECT_101)
__host__ __device__ inline int reflect101(int p, int n)
{
    if (n == 1)
        return 0;
    while ((unsigned)p >= (unsigned)n)
        p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

} // namespace lk
} // namespace tf
