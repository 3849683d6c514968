// Still pixmaps made in device memory (transflow/pixmap/still.py): a colour fill and the gradient's expression tree.
//
// GradientPixmapSource._init_array (still.py:151-163) walks a random tree of at most 40 nodes once per pixel, in
// Python.  Every operation of it is a float64 operation on the pixel's own (i, j): one thread per pixel does the same
// operations in the same order (-ffp-contract=off keeps each rounding) and the bytes are the reference's.
//
// No scratch: an evaluation stack indexed at run time would live in scratch memory.  The trees still.py:94-119 makes
// have ONE shape -- generate(TRIPLE, 5): a triple of three B(4); B(d) is a leaf or a mix of three B(d - 2); B(0) is a
// leaf -- and a mix works channel by channel, a triple picks channel k of its k-th child.  So output channel k is the
// value of a fixed 1 + 3 + 9 slot tree of scalars: the top slot a leaf or a mix of three middle slots, each of those
// a leaf or a mix of three leaves.  The host resolves the tree into that table (Plan, a kernel argument: its flags
// and constants are wave-uniform scalars), the kernel walks the table with constant indices.  Whether a slot is a mix
// or a leaf is a uniform branch; neither form changes a bit of what is computed.
//
// A thread owns 4 consecutive pixels of the flat image = 12 bytes = three whole dwords at a dword-aligned address
// whatever the width (a row of 53 pixels is 159 bytes); the last thread stores the 1-3 pixels of a tail by bytes.
#include "common.h"

namespace tf {
namespace px {

constexpr int BLOCK = 256;
constexpr int PX_PER_THREAD = 4;

enum { LEAF_I = 0, LEAF_J = 1, LEAF_CONST = 2 };

struct Leaf {
    int kind;
    double c;
};

// one output channel: top, 3 middle slots, 9 leaves
struct Chan {
    int top_mix, mid_mix[3];
    Leaf top, mid[3], leaf[9];
};

struct Plan {
    Chan ch[3];
};
static_assert(sizeof(Plan) <= 1024, "Plan travels as a kernel argument");

__device__ __forceinline__ double leaf_value(const Leaf &l, double zi, double zj)
{
    return l.kind == LEAF_I ? zi : (l.kind == LEAF_J ? zj : l.c);
}

// still.py:136-137
__device__ __forceinline__ double mix(double a, double b, double c)
{
    const double w = (1.0 + a) / 2.0;
    return (1.0 - w) * b + w * c;
}

__device__ __forceinline__ double channel_value(const Chan &ch, double zi, double zj)
{
    if (!ch.top_mix)
        return leaf_value(ch.top, zi, zj);
    double m[3];
#pragma unroll
    for (int s = 0; s < 3; s++) {
        if (ch.mid_mix[s])
            m[s] = mix(leaf_value(ch.leaf[3 * s], zi, zj), leaf_value(ch.leaf[3 * s + 1], zi, zj),
                       leaf_value(ch.leaf[3 * s + 2], zi, zj));
        else
            m[s] = leaf_value(ch.mid[s], zi, zj);
    }
    return mix(m[0], m[1], m[2]);
}

// still.py:160-162 and numpy's float64 -> uint8 store: truncation to a 32-bit integer, its low byte
__device__ __forceinline__ uint32_t channel_byte(double v)
{
    const double x = (255.0 * (v + 1.0)) / 2.0;
    return (uint32_t)(int32_t)x & 255u;
}

__global__ __launch_bounds__(BLOCK) void k_pixmap_gradient(uint8_t *__restrict__ rgb, uint32_t n, uint32_t W, FastDiv divW,
                                                          double hm1, double wm1, const Plan plan)
{
    const uint32_t p0 = (blockIdx.x * (uint32_t)BLOCK + threadIdx.x) * PX_PER_THREAD; // n < 2^31: no wrap
    if (p0 >= n)
        return;
    uint32_t b[3 * PX_PER_THREAD];
#pragma unroll
    for (int q = 0; q < PX_PER_THREAD; q++) {
        const uint32_t p = p0 + q; // (past the end in a tail: computed, never stored)
        const uint32_t i = fast_div(p, divW), j = p - i * W;
        const double zi = 2.0 * ((double)i / hm1) - 1.0; // still.py:144
        const double zj = 2.0 * ((double)j / wm1) - 1.0; // still.py:147
#pragma unroll
        for (int k = 0; k < 3; k++)
            b[3 * q + k] = channel_byte(channel_value(plan.ch[k], zi, zj));
    }
    if (p0 + PX_PER_THREAD <= n) {
        uint32_t *out = reinterpret_cast<uint32_t *>(rgb + (size_t)p0 * 3);
#pragma unroll
        for (int d = 0; d < 3; d++)
            out[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
    } else {
#pragma unroll
        for (int q = 0; q < PX_PER_THREAD - 1; q++)
            if (p0 + q < n) {
#pragma unroll
                for (int k = 0; k < 3; k++)
                    rgb[(size_t)(p0 + q) * 3 + k] = (uint8_t)b[3 * q + k];
            }
    }
}

// 4 pixels of one colour are the same three dwords everywhere
__global__ __launch_bounds__(BLOCK) void k_pixmap_fill(uint8_t *__restrict__ rgb, size_t n, uint32_t w0, uint32_t w1, uint32_t w2,
                                                      uint32_t r, uint32_t g, uint32_t b)
{
    const size_t p0 = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * PX_PER_THREAD;
    if (p0 >= n)
        return;
    if (p0 + PX_PER_THREAD <= n) {
        uint32_t *out = reinterpret_cast<uint32_t *>(rgb + p0 * 3);
        out[0] = w0, out[1] = w1, out[2] = w2;
    } else {
        for (size_t p = p0; p < n; p++)
            rgb[p * 3] = (uint8_t)r, rgb[p * 3 + 1] = (uint8_t)g, rgb[p * 3 + 2] = (uint8_t)b;
    }
}

// ---- host: postfix list -> tree -> Plan ----------------------------------------------------------------------------
struct HNode {
    int type;
    double v[3];
    int kid[3];
};

static bool is_leaf(int type) { return type == TF_PX_I || type == TF_PX_J || type == TF_PX_RGB; }

// channel k of a triple is channel k of its k-th child (still.py:123-127)
static int through_triples(const HNode *t, int node, int k)
{
    while (t[node].type == TF_PX_TRIPLE)
        node = t[node].kid[k];
    return node;
}

static Leaf leaf_of(const HNode &h, int k)
{
    Leaf l;
    l.kind = h.type == TF_PX_I ? LEAF_I : (h.type == TF_PX_J ? LEAF_J : LEAF_CONST);
    l.c = h.type == TF_PX_RGB ? h.v[k] : 0.0;
    return l;
}

static int make_plan(const tf_px_node *nodes, int n_nodes, int width, int height, Plan *plan)
{
    TF_REQUIRE(n_nodes >= 1 && n_nodes <= TF_PX_MAX_NODES, "tf_pixmap_gradient_dev: %d nodes (1 to %d)", n_nodes, TF_PX_MAX_NODES);
    HNode t[TF_PX_MAX_NODES];
    int stack[TF_PX_MAX_NODES], sp = 0;
    for (int n = 0; n < n_nodes; n++) {
        const tf_px_node &nd = nodes[n];
        TF_REQUIRE(is_leaf(nd.type) || nd.type == TF_PX_MIX || nd.type == TF_PX_TRIPLE,
                   "tf_pixmap_gradient_dev: node %d has unknown type %d", n, nd.type);
        // the reference evaluates every node for every pixel, also those a triple then drops (still.py:144, 147)
        TF_REQUIRE(!(nd.type == TF_PX_I && height == 1), "tf_pixmap_gradient_dev: division by zero (a row node, height 1)");
        TF_REQUIRE(!(nd.type == TF_PX_J && width == 1), "tf_pixmap_gradient_dev: division by zero (a column node, width 1)");
        t[n].type = nd.type;
        t[n].v[0] = nd.a, t[n].v[1] = nd.b, t[n].v[2] = nd.c;
        t[n].kid[0] = t[n].kid[1] = t[n].kid[2] = -1;
        if (!is_leaf(nd.type)) {
            TF_REQUIRE(sp >= 3, "tf_pixmap_gradient_dev: node %d needs three values below it, the postfix order gives %d", n, sp);
            for (int c = 2; c >= 0; c--)
                t[n].kid[c] = stack[--sp];
        }
        stack[sp++] = n;
    }
    TF_REQUIRE(sp == 1, "tf_pixmap_gradient_dev: the postfix order leaves %d trees, not one", sp);
    const int root = stack[0];
    *plan = Plan{};
    for (int k = 0; k < 3; k++) {
        Chan &ch = plan->ch[k];
        const int top = through_triples(t, root, k);
        if (is_leaf(t[top].type)) {
            ch.top = leaf_of(t[top], k);
            continue;
        }
        ch.top_mix = 1;
        for (int s = 0; s < 3; s++) {
            const int mid = through_triples(t, t[top].kid[s], k);
            if (is_leaf(t[mid].type)) {
                ch.mid[s] = leaf_of(t[mid], k);
                continue;
            }
            ch.mid_mix[s] = 1;
            for (int l = 0; l < 3; l++) {
                const int low = through_triples(t, t[mid].kid[l], k);
                if (!is_leaf(t[low].type))
                    return set_error(TF_ERR_UNSUPPORTED, "tf_pixmap_gradient_dev: mixes nested three deep (node %d): "
                                                         "not a tree GradientPixmapSource.generate makes", low);
                ch.leaf[3 * s + l] = leaf_of(t[low], k);
            }
        }
    }
    return TF_OK;
}

} // namespace px
} // namespace tf

using namespace tf;
using namespace tf::px;

TF_API int tf_pixmap_fill_dev(void *rgb_dev, size_t n_pixels, const uint8_t rgb[3])
{
    TF_REQUIRE(rgb && (rgb_dev || n_pixels == 0), "tf_pixmap_fill_dev: null pointer");
    TF_REQUIRE(((uintptr_t)rgb_dev & 3) == 0, "tf_pixmap_fill_dev: the pixmap must be 4-byte aligned");
    TF_REQUIRE(n_pixels < ((size_t)1 << 32), "tf_pixmap_fill_dev: %zu pixels", n_pixels);
    TF_TRY(ensure_init());
    const uint32_t c[3] = {rgb[0], rgb[1], rgb[2]};
    uint32_t w[3];
    for (int d = 0; d < 3; d++)
        w[d] = c[(4 * d) % 3] | (c[(4 * d + 1) % 3] << 8) | (c[(4 * d + 2) % 3] << 16) | (c[(4 * d + 3) % 3] << 24);
    return launch("pixmap_fill", k_pixmap_fill, dim3(cdiv(cdiv(n_pixels, PX_PER_THREAD), BLOCK)), dim3(BLOCK), 0,
                  (uint8_t *)rgb_dev, n_pixels, w[0], w[1], w[2], c[0], c[1], c[2]);
}

TF_API int tf_pixmap_gradient_dev(void *rgb_dev, int width, int height, int n_nodes, const tf_px_node *nodes)
{
    TF_REQUIRE(rgb_dev && nodes, "tf_pixmap_gradient_dev: null pointer");
    TF_REQUIRE(((uintptr_t)rgb_dev & 3) == 0, "tf_pixmap_gradient_dev: the pixmap must be 4-byte aligned");
    TF_REQUIRE(width >= 1 && height >= 1 && (long long)width * height < (1ll << 31), "tf_pixmap_gradient_dev: bad size %dx%d",
               width, height);
    Plan plan;
    TF_TRY(make_plan(nodes, n_nodes, width, height, &plan)); // everything is checked before anything is launched
    TF_TRY(ensure_init());
    const uint32_t n = (uint32_t)width * (uint32_t)height;
    // (a size-1 axis has no I / J node: make_plan refused it; the divisor is then never used)
    const double hm1 = height > 1 ? (double)(height - 1) : 1.0, wm1 = width > 1 ? (double)(width - 1) : 1.0;
    return launch("pixmap_gradient", k_pixmap_gradient, dim3(cdiv(cdiv(n, PX_PER_THREAD), BLOCK)), dim3(BLOCK), 0,
                  (uint8_t *)rgb_dev, n, (uint32_t)width, fast_div_setup((uint32_t)width), hm1, wm1, plan);
}
