// Horn-Schunck (transflow/flow/methods/horn_schunck.py): what hornschunck.hip and hs_norm.hip share.
#pragma once
#include "common.h"

#include <array>

namespace tf {
namespace hs {

constexpr int MAX_PAIRS = 64;      // pairs of one tf_hs_calc_slots call (descriptors travel as a kernel argument)
constexpr int IT_BX = 256;         // iteration kernel: one thread per column of a 256-column block ...
constexpr int IT_ROWS = 32;        // ... marching down a strip of 32 rows
constexpr double GUARD = 1e-3;     // relative guard of the spectral-norm test (covers LAPACK's rounding of sigma)
constexpr int POWER_STEPS = 8;     // power-iteration steps before the Gram certificate

enum Decision { UNDECIDED = -1, NOT_CONVERGED = 0, CONVERGED = 1 };
enum Stage { ST_BOUNDS = 0, ST_POWER = 1, ST_GRAM = 2, ST_HOST = 3, ST_COUNT = 4 };

// One active pair of a launch: its index and which of its two u/v buffers holds the current field.
struct PairDesc {
    int pair, cur;
};
struct PairList {
    int n;
    PairDesc p[MAX_PAIRS];
};

// Column partials of a strip: [2][n_strips][W] (sum of du^2, sum of |du|); row partials of a column block:
// [2][n_colblocks][H].  Per pair, partial_doubles apart.
__host__ __device__ inline int n_strips(int H) { return (H + IT_ROWS - 1) / IT_ROWS; }
__host__ __device__ inline int n_colblocks(int W) { return (W + IT_BX - 1) / IT_BX; }
inline size_t partial_doubles(int W, int H) { return 2 * ((size_t)n_strips(H) * W + (size_t)n_colblocks(W) * H); }
// the reduction kernel: one block per 256 columns and one per 256 rows, 4 doubles each
// {max of the sums of du^2, max of the sums of |du|, sum of du^2 (column blocks), non-finite sums}
inline int n_bound_blocks(int W, int H) { return (W + 255) / 256 + (H + 255) / 256; }

// Scratch of the spectral-norm test, sized for one W x H field; the Gram buffers are allocated on first use.
struct NormScratch {
    int W = 0, H = 0;
    DevBuf partials, blocks, pw_x, pw_y, pw_xpart, pw_scal, gram_a, gram_g, sums;
    std::vector<double> host_blocks;
    int init(int w, int h);
};

// The cheap bounds of one pair, from its reduced blocks.  nonfinite: du has a NaN or an inf (or a square that
// overflows).  tiny: ||du||_F^2 < TINY_F2, where the squares of du leave float64's normal range: F and L (sums of
// squares) are not used then and U is sqrt(n1) sqrt(ninf), the sums of |du| being exact at any magnitude.  In both
// cases the device stages after the bounds are not run: what the bounds cannot decide goes to the host.
constexpr double TINY_F2 = 0x1p-960;
struct Bounds {
    double F, U, L;
    bool nonfinite, tiny;
    bool device_stages() const { return !nonfinite && !tiny; }
};
Bounds bounds_of(const double *blocks, int W, int H);
// -> CONVERGED / NOT_CONVERGED / UNDECIDED
int decide_bounds(const Bounds &b, double delta);
// What the device stages after the bounds compute for one pair: the lower bounds of the power iteration (two per
// step) and the upper bounds of the Gram certificate (k = 1, 2, 4; NaN where F is zero).
struct StageValues {
    double power[2 * POWER_STEPS], gram[3];
};
// every stage without early exit
int device_values(NormScratch &s, const void *u_new, const void *u_old, bool f64, double F, StageValues *v);
// the same stages, each decided as soon as its values are read back.  Returns the decision and the stage that made
// it (ST_HOST if neither could).
int decide_device(NormScratch &s, const void *u_new, const void *u_old, bool f64, double delta, double F, int *decision,
                  int *stage);
// enqueue the reduction of a launch's partials into blocks[n_active][n_bound_blocks][4]
int launch_bounds_reduce(const double *partials_base, size_t partials_stride, const PairList &pl, int W, int H,
                         double *blocks_out);
// column/row partials of du = u_new - u_old alone (the stage entry point; the iteration kernel fuses them)
int launch_delta_partials(const void *u_new, const void *u_old, bool f64, int W, int H, double *partials);
// du = u_new - u_old in the chain's type, into dst
int launch_delta(const void *u_new, const void *u_old, bool f64, size_t n, void *dst);

// Sum over the 64 lanes of a wave (lane 0's result is what is used: the same tree every time).
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o);
    return v;
}

// End of a 256 x IT_ROWS strip: the column sums of the thread (c < 0: a thread past the right edge) and the block's
// row sums (four wave sums per row in rowred, added in wave order) go to the pair's partials P.
__device__ __forceinline__ void strip_store(double *P, int W, int H, int c, int strip, int cb, int r0, int nrows, double csq,
                                            double cab, const double (*rowred)[4][2])
{
    const size_t S = (size_t)n_strips(H), CB = (size_t)n_colblocks(W);
    if (c >= 0) {
        P[(size_t)strip * W + c] = csq;
        P[S * W + (size_t)strip * W + c] = cab;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 2 * nrows) {
        const int rl = t >> 1, q = t & 1;
        const double s = ((rowred[rl][0][q] + rowred[rl][1][q]) + rowred[rl][2][q]) + rowred[rl][3][q];
        P[2 * S * W + q * CB * H + (size_t)cb * H + r0 + rl] = s;
    }
}

} // namespace hs
} // namespace tf

// the handle (include/tfhip.h)
struct tf_hs {
    int W = 0, H = 0, slots = 0, max_pairs = 0;
    tf::DevBuf frames;        // [slots][H][W] uint8
    tf::DevBuf bgr_stage;     // tf_hs_set_frame_bgr: the decoded frame on its way to a slot
    tf::DevBuf deriv;         // [max_pairs][H][W] float4 {ex, ey, et, den}
    tf::DevBuf uv;            // [max_pairs][2 buffers][2 planes u, v][H][W], 8 bytes per value (float or double)
    tf::DevBuf init_flow;     // [max_pairs][H][W][2] float: tf_hs_set_initial_flow
    tf::DevBuf flow;          // [max_pairs][H][W][2] float: the results
    tf::DevBuf partials;      // [max_pairs][partial_doubles]
    tf::DevBuf blocks;        // [max_pairs][n_bound_blocks][4]
    tf::hs::NormScratch norm;
    std::vector<double> host_blocks;
    std::vector<int> has_init;               // per pair: an initial flow was set for the next call (float32 chain)
    std::vector<const void *> init_dev;      // per pair: where that flow sits if not in init_flow (tf_hs_set_initial_flow_dev)
    // the call in progress
    tf_hs_params prm{};
    int n_pairs = 0, last_pairs = 0;
    enum State { RUNNING = 0, DONE = 1, WAITING = 2 };
    std::vector<int> state, iter, cur, f64;
    std::vector<std::array<int, 5>> stats;   // iterations, decisions by bounds, power, Gram, host
    size_t plane_bytes() const { return (size_t)W * H * 8; }
    void *plane(int pair, int buf, int comp) const
    {
        return (char *)uv.p + (((size_t)pair * 2 + buf) * 2 + comp) * plane_bytes();
    }
};
