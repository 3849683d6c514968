// Codec motion vectors painted into a flow (transflow/flow/sources/av.py:61-77): what the host arithmetic and the two
// kernels of motionvectors.hip share.
#pragma once
#include "common.h"

namespace tf {
namespace mv {

constexpr int PAINT_WAVES = 4;     // paint kernel: one wave per rectangle, four of them to a block
constexpr int RESOLVE_BX = 256;    // resolve kernel: one thread per pixel

// A rectangle that paints something, after numpy's slice resolution: rows [i0, i1) x columns [j0, j1), inside the frame.
struct Rect {
    int32_t i0, i1, j0, j1;
};

// One bound pair of a numpy basic slice a:b over an axis of length n (step 1): a negative bound counts from the end,
// then both are clamped to [0, n].  The painted range is [*lo, *hi), empty when *lo >= *hi.
inline void resolve_slice(long long a, long long b, long long n, int32_t *lo, int32_t *hi)
{
    if (a < 0)
        a += n;
    if (b < 0)
        b += n;
    a = a < 0 ? 0 : (a > n ? n : a);
    b = b < 0 ? 0 : (b > n ? n : b);
    *lo = (int32_t)a, *hi = (int32_t)b;
}

// Python's x // 2 (floor, also for a negative x)
inline long long floor_half(long long x) { return x >> 1; }

} // namespace mv
} // namespace tf

// the handle (include/tfhip.h)
struct tf_mv {
    int W = 0, H = 0;
    tf::DevBuf winner;        // [H][W] uint32: 1 + the index (among the painting rectangles) of the last writer, 0 = none
    tf::DevBuf table;         // [dev_cap] {Rect, value}: the painting rectangles of the frame, grows on demand
    tf::DevBuf flow;          // [H][W][2] float: tf_mv_rasterize's result on its way down (allocated on first use)
    tf::PinnedBuf stage;      // page-locked host image of the table for the upload
    size_t stage_cap = 0, dev_cap = 0;       // in rectangles
    tf::Event uploaded;                      // the last upload has left the stage
    bool dirty = false;       // a call failed between its two launches: the winner map is cleared before the next one
};
