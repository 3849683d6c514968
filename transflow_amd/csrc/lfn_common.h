// LiteFlowNet (transflow/flow/methods/liteflownet.py): what liteflownet.hip's kernels and its host code share.  The
// layer table mirrors transflow_amd/liteflownet.py layers(): the weight blob of tf_lfn_set_weights is every layer's
// weight [Cout][Cin][kh][kw] (transposed convs: [C][1][4][4]) and bias [Cout], one layer after another, in that order.
#pragma once
#include "common.h"

namespace tf {
namespace lfn {

constexpr int MAX_PAIRS = TF_LFN_MAX_PAIRS;
constexpr int N_LEVELS = 5;                                   // levels 2..6 (feature index level - 1)
constexpr int UNFOLD[7] = {0, 0, 7, 5, 5, 3, 3};
constexpr float BACKWARP[7] = {0.f, 0.f, 10.0f, 5.0f, 2.5f, 1.25f, 0.625f};
constexpr int FEAT_C[6] = {32, 32, 64, 96, 128, 192};
constexpr int SUB_CIN[7] = {0, 0, 130, 130, 194, 258, 386};
constexpr int REG_CIN[7] = {0, 0, 131, 131, 131, 131, 195};
constexpr float MEAN[2][3] = {{0.411618f, 0.434631f, 0.454253f}, {0.410782f, 0.433645f, 0.452793f}};

// Which profiler label a convolution carries (tools/bench_lfn.py sums FLOPs by these classes).
enum ConvClass { CC_7X7 = 0, CC_3X3_S1, CC_3X3_S2, CC_1X1, CC_KX1, CC_1XK, CC_HEAD, CC_DIST, CC_COUNT };

struct Layer {
    int cout, cin, kh, kw, stride, ph, pw, leaky, deconv;
    long long w_off, b_off; // float offsets into the blob (b_off -1: no bias)
    int nt, npad;           // MFMA N tiles of 32 per block, Cout padded to a multiple of 32 * nt
    long long pk_off;       // float offset of the packed [K][npad] weights (convolutions)
    int cls;
    int kpad;               // K rounded up to QCONV_BK: the row length of the layer's bf16 weights [npad][kpad]
    long long q_off;        // element offset of those rows in a bf16 plane (hi and lo planes share the layout)
};

// One convolution launch (k_lfn_conv, liteflownet.hip; k_lfn_conv_q, lfn_conv_bf16.hip).
struct ConvArgs {
    const float *in;     // [n][hin][win][in_cs], the layer's input channels at in_off ...
    const float *wt;     // packed [K][npad], K ordered (ky, kx, ci)
    const float *bias;   // [cout]
    float *out;          // [n][ho][wo][out_cs], written at out_off ...
    const float *res;    // optional residual [n][ho][wo][res_cs] at res_off
    int in_cs, in_off, out_cs, out_off, res_cs, res_off;
    int hin, win, ho, wo, M;
    int cin, cout, kh, kw, stride, ph, pw, K, npad, leaky;
};

constexpr int QCONV_BK = 32;  // the bf16 kernel's K chunk: two k-steps of v_mfma_f32_32x32x16_bf16

// lfn_conv_bf16.hip: the convolution of the bf16 (passes 1) and bf16x3 (passes 3) modes on the layer's bf16 weight
// planes, and the repack of a layer's float32 weights [Cout][Cin][kh][kw] into them.
// (name_vec: the launch's profiler label when it gathers with 128-bit loads, name otherwise)
int launch_conv_q(const char *name, const char *name_vec, const ConvArgs &a, const uint16_t *w_hi, const uint16_t *w_lo,
                  int kpad, int nt, int passes);
int pack_weights_q(const Layer &l, const float *w, uint16_t *hi, uint16_t *lo);

// Indices of the layers the driver runs, per level (index 0 = level 2); -1 where the level has none.
struct LevelLayers {
    int m_feat, m_upflow, m_upcorr, m_main[4];
    int s_feat, s_main[4];
    int r_feat, r_main[6], r_dist0, r_dist1, r_scale_x, r_scale_y;
};

struct Net {
    std::vector<Layer> layers;
    int feat[10];                 // the ten convolutions of the feature pyramid
    LevelLayers lv[N_LEVELS];
    long long blob_floats, packed_floats, q_elems;
};

inline Net make_net()
{
    Net net{};
    long long off = 0;
    auto add = [&](int cout, int cin, int kh, int kw, int stride, int leaky, int deconv) {
        Layer l{};
        l.cout = cout, l.cin = cin, l.kh = kh, l.kw = kw, l.stride = stride, l.ph = (kh - 1) / 2, l.pw = (kw - 1) / 2;
        l.leaky = leaky, l.deconv = deconv;
        l.w_off = off;
        off += deconv ? (long long)cout * 16 : (long long)cout * cin * kh * kw;
        l.b_off = -1;
        if (!deconv) {
            l.b_off = off;
            off += cout;
        }
        net.layers.push_back(l);
        return (int)net.layers.size() - 1;
    };
    auto conv = [&](int cout, int cin, int k, int stride = 1, int leaky = 1) { return add(cout, cin, k, k, stride, leaky, 0); };
    const int fdesc[10][4] = {{32, 3, 7, 1},  {32, 32, 3, 2}, {32, 32, 3, 1}, {32, 32, 3, 1},   {64, 32, 3, 2},
                              {64, 64, 3, 1}, {96, 64, 3, 2}, {96, 96, 3, 1}, {128, 96, 3, 2}, {192, 128, 3, 2}};
    for (int i = 0; i < 10; i++)
        net.feat[i] = conv(fdesc[i][0], fdesc[i][1], fdesc[i][2], fdesc[i][3]);
    for (int i = 0; i < N_LEVELS; i++) {
        const int L = i + 2, k = UNFOLD[L];
        LevelLayers &v = net.lv[i];
        v.m_feat = L == 2 ? conv(64, 32, 1) : -1;
        v.m_upflow = L != 6 ? add(2, 2, 4, 4, 2, 0, 1) : -1;
        v.m_upcorr = L < 4 ? add(49, 49, 4, 4, 2, 0, 1) : -1;
        v.m_main[0] = conv(128, 49, 3);
        v.m_main[1] = conv(64, 128, 3);
        v.m_main[2] = conv(32, 64, 3);
        v.m_main[3] = conv(2, 32, k, 1, 0);
    }
    for (int i = 0; i < N_LEVELS; i++) {
        const int L = i + 2, k = UNFOLD[L];
        LevelLayers &v = net.lv[i];
        v.s_feat = L == 2 ? conv(64, 32, 1) : -1;
        v.s_main[0] = conv(128, SUB_CIN[L], 3);
        v.s_main[1] = conv(64, 128, 3);
        v.s_main[2] = conv(32, 64, 3);
        v.s_main[3] = conv(2, 32, k, 1, 0);
    }
    for (int i = 0; i < N_LEVELS; i++) {
        const int L = i + 2, k = UNFOLD[L];
        LevelLayers &v = net.lv[i];
        v.r_feat = L < 5 ? conv(128, FEAT_C[L - 1], 1) : -1;
        const int mc[6][2] = {{128, REG_CIN[L]}, {128, 128}, {64, 128}, {64, 64}, {32, 64}, {32, 32}};
        for (int j = 0; j < 6; j++)
            v.r_main[j] = conv(mc[j][0], mc[j][1], 3);
        if (L < 5) {
            v.r_dist0 = add(k * k, 32, k, 1, 1, 0, 0);
            v.r_dist1 = add(k * k, k * k, 1, k, 1, 0, 0);
        } else {
            v.r_dist0 = conv(k * k, 32, k, 1, 0);
            v.r_dist1 = -1;
        }
        v.r_scale_x = conv(1, k * k, 1, 1, 0);
        v.r_scale_y = conv(1, k * k, 1, 1, 0);
    }
    net.blob_floats = off;
    long long pk = 0;
    for (size_t i = 0; i < net.layers.size(); i++) {
        Layer &l = net.layers[i];
        if (l.deconv)
            continue;
        const int t = (l.cout + 31) / 32;
        l.nt = t <= 4 ? t : l.cout % 128 == 0 ? 4 : l.cout % 96 == 0 ? 3 : l.cout % 64 == 0 ? 2 : 4;
        l.npad = (l.cout + 32 * l.nt - 1) / (32 * l.nt) * (32 * l.nt);
        l.pk_off = pk;
        pk += (long long)l.kh * l.kw * l.cin * l.npad;
        l.cls = l.cout == 2                  ? CC_HEAD
                : l.kh == 1 && l.kw == 1     ? CC_1X1
                : l.kw == 1                  ? CC_KX1
                : l.kh == 1                  ? CC_1XK
                : l.kh == 7 && l.cin == 3    ? CC_7X7
                : l.cout == l.kh * l.kw      ? CC_DIST
                : l.stride == 2              ? CC_3X3_S2
                                             : CC_3X3_S1;
    }
    net.packed_floats = pk;
    long long q = 0;
    for (Layer &l : net.layers) {
        if (l.deconv)
            continue;
        l.kpad = (l.kh * l.kw * l.cin + QCONV_BK - 1) / QCONV_BK * QCONV_BK;
        l.q_off = q;
        q += (long long)l.npad * l.kpad;
    }
    net.q_elems = q;
    return net;
}

} // namespace lfn
} // namespace tf
