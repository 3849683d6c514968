// Codec motion vectors -> flow (transflow/flow/sources/av.py:61-77).  The reference starts from zeros and, for each
// vector in list order, assigns (-motion_x / motion_scale, -motion_y / motion_scale) to the numpy slice
// flow[src_y - h//2 : src_y + h//2, src_x - w//2 : src_x + w//2]: rectangles overlap freely and the last writer wins.
//
// Here the slice resolution, the division and the validation run on the host (resolve_vector below: a few integer
// operations and two divisions per vector); rectangles that paint nothing are dropped, which keeps the order of the
// others.  The device gets the table of the rest and does two launches:
//   mv_paint    one wave per rectangle: atomicMax(winner[p], 1 + index) over its pixels.  A maximum does not depend on
//               the order of arrival, so the winner map -- and the flow -- is the same on every run.
//   mv_resolve  one thread per pixel: flow[p] = value of winner[p] (or +0, +0), one 8-byte store, and winner[p] goes back
//               to 0, so the next frame starts from a clean map without a memset.
// The same form as k_pp_fwd_scatter / k_pp_fwd_resolve (postprocess.hip).
#include "mv_common.h"

#include <new>

namespace tf {
namespace mv {

// What travels to the device per painting rectangle: 24 bytes, the value 8-byte aligned.
struct Item {
    Rect r;
    float vx, vy;
};
static_assert(sizeof(Item) == 24, "Item layout");

// av.py:69-76 for one vector: the assert, the four bounds through numpy's slice resolution, the two divisions (Python
// int / int is the correctly rounded float64 quotient; the assignment rounds it to float32).
static int resolve_vector(const char *who, int W, int H, const tf_mv_vector &v, int index, Rect *r, float *val)
{
    TF_REQUIRE(v.source == -1, "%s: vector %d has source %d, not -1 (encode with bf=0 and refs=1)", who, index, v.source);
    TF_REQUIRE(v.motion_scale != 0, "%s: vector %d has motion_scale 0", who, index);
    const long long hh = floor_half(v.h), hw = floor_half(v.w);
    resolve_slice((long long)v.src_y - hh, (long long)v.src_y + hh, H, &r->i0, &r->i1);
    resolve_slice((long long)v.src_x - hw, (long long)v.src_x + hw, W, &r->j0, &r->j1);
    const double dx = (double)v.motion_x / (double)v.motion_scale, dy = (double)v.motion_y / (double)v.motion_scale;
    val[0] = (float)-dx, val[1] = (float)-dy;
    return TF_OK;
}

// One wave per rectangle, lanes along j: a row segment takes the smallest power of two of lanes that holds it (at most
// 64) and the wave covers 64 / that many rows per instruction -- a 16-wide partition is four 64-byte segments, anything
// from 33 columns up whole 256-byte rows.  Rectangles lie inside the frame (resolve_slice clamps to [0, n]).
__global__ __launch_bounds__(PAINT_WAVES * 64) void k_mv_paint(const Item *__restrict__ items, int n,
                                                               uint32_t *__restrict__ winner, int W)
{
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * PAINT_WAVES + (threadIdx.x >> 6);
    if (k >= n)
        return;
    const Rect r = items[k].r;
    const int cw = r.j1 - r.j0;
    int lsh = 6;
    while (lsh > 0 && (1 << (lsh - 1)) >= cw)
        lsh--;
    const int lw = 1 << lsh, rows = 64 >> lsh;
    const uint32_t id = (uint32_t)k + 1u;
    for (int j = r.j0 + (lane & (lw - 1)); j < r.j1; j += lw)
        for (int i = r.i0 + (lane >> lsh); i < r.i1; i += rows)
            (void)__hip_atomic_fetch_max(&winner[(size_t)i * W + j], id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(RESOLVE_BX) void k_mv_resolve(uint32_t *__restrict__ winner, const Item *__restrict__ items,
                                                           int n, float2 *__restrict__ flow, int N)
{
    const uint32_t p = blockIdx.x * (uint32_t)RESOLVE_BX + threadIdx.x;      // N < 2^31: no wrap in the last block
    if (p >= (uint32_t)N)
        return;
    const uint32_t w = winner[p];
    float2 v = make_float2(0.0f, 0.0f);
    if (w) {
        if (w <= (uint32_t)n)      // (always, with a clean map: never read past the table)
            v = make_float2(items[w - 1].vx, items[w - 1].vy);
        winner[p] = 0;
    }
    flow[p] = v;
}

// The stage holds the table on its way up; it is written again only once the previous upload has left it.  One stage,
// not two: the host loop over frame N + 1 starts after frame N's upload (a few MB) has ended, never beside it.
static int reserve(tf_mv *mv, size_t n)
{
    if (mv->uploaded)
        TF_HIP(hipEventSynchronize(mv->uploaded));
    if (n > mv->stage_cap) {
        const size_t cap = n + n / 2 + 1024;
        mv->stage.release();
        mv->stage_cap = 0;
        TF_TRY(mv->stage.alloc(cap * sizeof(Item)));
        mv->stage_cap = cap;
    }
    return TF_OK;
}

static int clear_map(tf_mv *mv)
{
    TF_HIP(hipMemsetAsync(mv->winner.p, 0, mv->winner.bytes, stream()));
    mv->dirty = false;
    return TF_OK;
}

static int rasterize(tf_mv *mv, const tf_mv_vector *v, int n, float2 *flow_dev)
{
    TF_TRY(ensure_init());
    TF_TRY(reserve(mv, (size_t)n));
    Item *items = mv->stage.as<Item>();
    int m = 0;
    for (int k = 0; k < n; k++) {          // every vector is checked before anything is launched
        Rect r;
        float val[2];
        TF_TRY(resolve_vector("tf_mv_rasterize", mv->W, mv->H, v[k], k, &r, val));
        if (r.i0 < r.i1 && r.j0 < r.j1)
            items[m++] = Item{r, val[0], val[1]};
    }
    if ((size_t)m > mv->dev_cap) {
        mv->dev_cap = 0;
        TF_TRY(mv->table.alloc(mv->stage_cap * sizeof(Item)));
        mv->dev_cap = mv->stage_cap;
    }
    if (mv->dirty)
        TF_TRY(clear_map(mv));
    if (m > 0) {
        TF_HIP(hipMemcpyAsync(mv->table.p, items, (size_t)m * sizeof(Item), hipMemcpyHostToDevice, stream()));
        TF_HIP(hipEventRecord(mv->uploaded, stream()));
    }
    const int N = mv->W * mv->H;
    mv->dirty = true;                      // until both launches are on their way
    TF_TRY(launch("mv_paint", k_mv_paint, dim3(cdiv((size_t)m, PAINT_WAVES)), dim3(PAINT_WAVES * 64), 0,
                  (const Item *)mv->table.p, m, mv->winner.as<uint32_t>(), mv->W));
    TF_TRY(launch("mv_resolve", k_mv_resolve, dim3(cdiv((size_t)N, RESOLVE_BX)), dim3(RESOLVE_BX), 0,
                  mv->winner.as<uint32_t>(), (const Item *)mv->table.p, m, flow_dev, N));
    mv->dirty = false;
    return TF_OK;
}

} // namespace mv
} // namespace tf

using namespace tf;
using namespace tf::mv;

TF_API int tf_mv_create(tf_mv **out, int width, int height)
{
    TF_REQUIRE(out, "tf_mv_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(width >= 1 && height >= 1 && (long long)width * height < (1ll << 31), "tf_mv_create: bad size %dx%d", width,
               height);
    TF_TRY(ensure_init());
    auto mv = make_handle(tf_mv_destroy); // synchronises first: a failure may come after the clear was queued
    TF_REQUIRE(mv, "tf_mv_create: out of memory");
    mv->W = width, mv->H = height;
    TF_TRY(mv->winner.alloc((size_t)width * height * sizeof(uint32_t)));
    TF_TRY(mv->uploaded.create());
    TF_TRY(clear_map(mv.get())); // the one clear: mv_resolve leaves the map clean behind it
    *out = mv.release();
    return TF_OK;
}

TF_API void tf_mv_destroy(tf_mv *mv)
{
    if (!mv)
        return;
    (void)hipStreamSynchronize(stream()); // kernels of the handle's last call may still read its buffers
    delete mv;
}

TF_API int tf_mv_rasterize_dev(tf_mv *mv, const tf_mv_vector *v, int n, void *flow_dev)
{
    TF_REQUIRE(mv && flow_dev, "tf_mv_rasterize_dev: null pointer");
    TF_REQUIRE(n >= 0 && (v || n == 0), "tf_mv_rasterize_dev: %d vectors at a null pointer", n);
    TF_REQUIRE(((uintptr_t)flow_dev & 7) == 0, "tf_mv_rasterize_dev: the flow must be 8-byte aligned");
    return rasterize(mv, v, n, (float2 *)flow_dev);
}

TF_API int tf_mv_rasterize(tf_mv *mv, const tf_mv_vector *v, int n, float *flow_out)
{
    TF_REQUIRE(mv && flow_out, "tf_mv_rasterize: null pointer");
    TF_REQUIRE(n >= 0 && (v || n == 0), "tf_mv_rasterize: %d vectors at a null pointer", n);
    const size_t bytes = (size_t)mv->W * mv->H * sizeof(float2);
    if (!mv->flow.p)
        TF_TRY(mv->flow.alloc(bytes));
    TF_TRY(rasterize(mv, v, n, mv->flow.as<float2>()));
    TF_HIP(hipMemcpyAsync(flow_out, mv->flow.p, bytes, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

// Host arithmetic only (no device is touched): every vector's resolved slice bounds, empty ones as they come out
// (i0 >= i1 or j0 >= j1), and its value.
TF_API int tf_mv_stage_resolve_rects(int width, int height, const tf_mv_vector *v, int n, int32_t *rects_out, float *values_out)
{
    TF_REQUIRE(width >= 1 && height >= 1, "tf_mv_stage_resolve_rects: bad size %dx%d", width, height);
    TF_REQUIRE(n >= 0 && ((v && rects_out && values_out) || n == 0), "tf_mv_stage_resolve_rects: null pointer");
    for (int k = 0; k < n; k++) {
        Rect r;
        TF_TRY(resolve_vector("tf_mv_stage_resolve_rects", width, height, v[k], k, &r, values_out + 2 * (size_t)k));
        int32_t *o = rects_out + 4 * (size_t)k;
        o[0] = r.i0, o[1] = r.i1, o[2] = r.j0, o[3] = r.j1;
    }
    return TF_OK;
}
