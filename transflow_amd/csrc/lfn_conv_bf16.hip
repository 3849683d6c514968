// LiteFlowNet's convolutions in the bf16 and bf16x3 precision modes (tf_lfn_set_precision): the same implicit GEMM as
// k_lfn_conv (liteflownet.hip) -- M = output pixels of all images, N = Cout, K = kh kw Cin ordered (ky, kx, ci), bias,
// LeakyReLU and the residual in a float32 epilogue, channel slices of NHWC buffers in and out -- on
// v_mfma_f32_32x32x16_bf16.
//
// With q(v) = v rounded to bfloat16, ties to even:
//   bf16     every output is  sum_k q(x_k) q(w_k) + b
//   bf16x3   with xh = q(x), xl = q(x - xh), wh = q(w), wl = q(w - wh):
//            sum_k (xh_k wh_k + xh_k wl_k + xl_k wh_k) + b
// A product of two bf16 values is exact in float32; the sum is float32.  Every output is ONE accumulator chain over K
// in ascending order, 16 k per MFMA; in bf16x3 the chain takes, for each step of 16 k, xh wh, then xh wl, then xl wh.
// No split K and no atomics: flows are bit-identical from run to run and a pair in a batch equals the pair alone.
//
// Activations stay float32 in HBM and are rounded on their way into LDS, so LDS holds bf16 (and, for bf16x3, the lo
// plane beside it); the weights are rounded once, by k_lfn_pack_q, into hi and lo planes [npad][kpad] with K padded
// to the K chunk with zeros and K contiguous, so that a lane's MFMA fragment of either operand (8 consecutive k of
// one row) is one 16-byte LDS read.
#include "lfn_common.h"

namespace tf {
namespace lfn {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int Q_BM = 128, Q_THREADS = 256;
// LDS rows of QCONV_BK bf16 padded to 40 (80 bytes): 16-byte aligned, and the 16 rows a quarter wave reads start in
// 16 different groups of 4 banks
constexpr int Q_LD = QCONV_BK + 8;

struct QConvArgs {
    ConvArgs a;                 // (a.wt is not used)
    const uint16_t *wh, *wl;    // the layer's bf16 weight planes [npad][kpad]
    int kpad;
};

__device__ __forceinline__ float lrelu_q(float v) { return v > 0.f ? v : v * 0.1f; }

// float32 -> bfloat16, ties to even (v_cvt_pk_bf16_f32 on gfx950), as its 16 bits
__device__ __forceinline__ uint32_t bf16_bits(float v) { return (uint32_t)__builtin_bit_cast(unsigned short, (__bf16)v); }
__device__ __forceinline__ float bf16_value(float v) { return (float)(__bf16)v; }

// 4 floats -> 4 bf16 in 8 bytes (hi), and the bf16 of what the rounding left (lo)
template <bool LO>
__device__ __forceinline__ void split4(const float4 v, uint2 &hi, uint2 &lo)
{
    hi.x = bf16_bits(v.x) | (bf16_bits(v.y) << 16);
    hi.y = bf16_bits(v.z) | (bf16_bits(v.w) << 16);
    if (LO) {
        lo.x = bf16_bits(v.x - bf16_value(v.x)) | (bf16_bits(v.y - bf16_value(v.y)) << 16);
        lo.y = bf16_bits(v.z - bf16_value(v.z)) | (bf16_bits(v.w - bf16_value(v.w)) << 16);
    }
}

// Block: 128 output pixels x 32 NT channels, 4 waves of 32 pixels each.  Per K chunk of 32 the block stages A (the
// im2col rows, gathered with zero padding and rounded) and B (the bf16 weights) in LDS, and each wave runs 2 k-steps
// of NT (bf16) or 3 NT (bf16x3) 32x32x16 MFMAs.  Thread t gathers the 4 K columns 4 (t % 8) ... of pixels t / 8 + 32 p
// (p = 0..3): with VEC (Cin, the slice's offset and the buffer's channel stride all multiples of 4, so the four are
// neighbouring channels of one tap, 16-byte aligned) as one 128-bit load, otherwise one by one.  The chunks are
// double-buffered: the next chunk's global loads are issued before the MFMAs of the current one and land in the other
// LDS buffer after them, one barrier per chunk.
template <int NT, int PASSES, bool VEC>
__global__ __launch_bounds__(Q_THREADS) void k_lfn_conv_q(QConvArgs q)
{
    constexpr int BN = 32 * NT, PL = PASSES == 3 ? 2 : 1;
    constexpr int BLD = (BN * 4 + Q_THREADS - 1) / Q_THREADS; // 16-byte weight loads per thread and plane
    __shared__ __attribute__((aligned(16))) uint16_t As[2][PL][Q_BM][Q_LD];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][PL][BN][Q_LD];
    const ConvArgs &a = q.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * Q_BM, n0 = blockIdx.y * BN;
    const int kg = tid & 7, pr = tid >> 3;
    const float *base[4];
    int iy0[4], ix0[4];
    const int hw = a.ho * a.wo;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const int m = m0 + pr + 32 * p;
        base[p] = nullptr;
        iy0[p] = ix0[p] = 0;
        if (m < a.M) {
            const int b = m / hw, r = m - b * hw, oy = r / a.wo, ox = r - oy * a.wo;
            base[p] = a.in + (size_t)b * a.hin * a.win * a.in_cs + a.in_off;
            iy0[p] = oy * a.stride - a.ph, ix0[p] = ox * a.stride - a.pw;
        }
    }
    float4 ra[4];
    u32x4 rbh[BLD], rbl[PL == 2 ? BLD : 1];

    // chunk k0's operands from global memory into registers
    auto load = [&](int k0) __attribute__((always_inline)) {
        const int k = k0 + 4 * kg;
        int tap = k / a.cin, ci = k - tap * a.cin;
        int ky = tap / a.kw, kx = tap - ky * a.kw;
        if (VEC) {
            const bool kval = k < a.K;
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int iy = iy0[p] + ky, ix = ix0[p] + kx;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kval && base[p] && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win)
                    v = *reinterpret_cast<const float4 *>(base[p] + ((size_t)iy * a.win + ix) * a.in_cs + ci);
                ra[p] = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool kval = k + j < a.K;
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int iy = iy0[p] + ky, ix = ix0[p] + kx;
                    float v = 0.f;
                    if (kval && base[p] && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win)
                        v = base[p][((size_t)iy * a.win + ix) * a.in_cs + ci];
                    (&ra[p].x)[j] = v;
                }
                if (++ci == a.cin) {
                    ci = 0;
                    if (++kx == a.kw)
                        kx = 0, ky++;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < BLD; i++) {
            const int e = tid + Q_THREADS * i;
            if (BN * 4 % Q_THREADS == 0 || e < BN * 4) {
                const size_t at = (size_t)(n0 + (e >> 2)) * q.kpad + k0 + 8 * (e & 3);
                rbh[i] = *reinterpret_cast<const u32x4 *>(q.wh + at);
                if (PL == 2)
                    rbl[i] = *reinterpret_cast<const u32x4 *>(q.wl + at);
            }
        }
    };
    // ... rounded, into LDS buffer s
    auto store = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 4; p++) {
            uint2 hi, lo;
            split4<PL == 2>(ra[p], hi, lo);
            *reinterpret_cast<uint2 *>(&As[s][0][pr + 32 * p][4 * kg]) = hi;
            if (PL == 2)
                *reinterpret_cast<uint2 *>(&As[s][PL - 1][pr + 32 * p][4 * kg]) = lo;
        }
#pragma unroll
        for (int i = 0; i < BLD; i++) {
            const int e = tid + Q_THREADS * i;
            if (BN * 4 % Q_THREADS == 0 || e < BN * 4) {
                *reinterpret_cast<u32x4 *>(&Bs[s][0][e >> 2][8 * (e & 3)]) = rbh[i];
                if (PL == 2)
                    *reinterpret_cast<u32x4 *>(&Bs[s][PL - 1][e >> 2][8 * (e & 3)]) = rbl[i];
            }
        }
    };

    floatx16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
        for (int r = 0; r < 16; r++)
            acc[t][r] = 0.f;
    const int nchunks = q.kpad / QCONV_BK;
    load(0);
    for (int c = 0; c < nchunks; c++) {
        const int s = c & 1;
        store(s);
        __syncthreads();
        if (c + 1 < nchunks)
            load((c + 1) * QCONV_BK);
#pragma unroll
        for (int ks = 0; ks < QCONV_BK / 16; ks++) {
            const int ko = ks * 16 + 8 * (lane >> 5);
            const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(&As[s][0][wave * 32 + (lane & 31)][ko]);
            bf16x8 al = ah;
            if (PASSES == 3)
                al = *reinterpret_cast<const bf16x8 *>(&As[s][PL - 1][wave * 32 + (lane & 31)][ko]);
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const bf16x8 bh = *reinterpret_cast<const bf16x8 *>(&Bs[s][0][t * 32 + (lane & 31)][ko]);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t], 0, 0, 0);
                if (PASSES == 3) {
                    const bf16x8 bl = *reinterpret_cast<const bf16x8 *>(&Bs[s][PL - 1][t * 32 + (lane & 31)][ko]);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[t], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int n = n0 + t * 32 + (lane & 31);
        if (n >= a.cout)
            continue;
        const float b = a.bias[n];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m >= a.M)
                continue;
            float v = acc[t][r] + b;
            if (a.leaky)
                v = lrelu_q(v);
            if (a.res)
                v = a.res[(size_t)m * a.res_cs + a.res_off + n] + v;
            a.out[(size_t)m * a.out_cs + a.out_off + n] = v;
        }
    }
}

// [Cout][Cin][kh][kw] -> hi and lo planes [npad][kpad], k = (ky kw + kx) Cin + ci; zeros past Cout and past K
__global__ void k_lfn_pack_q(const float *__restrict__ w, uint16_t *__restrict__ hi, uint16_t *__restrict__ lo, int cout,
                             int cin, int kh, int kw, int npad, int kpad)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)npad * kpad)
        return;
    const int k = (int)(t % kpad), n = (int)(t / kpad);
    float v = 0.f;
    if (n < cout && k < kh * kw * cin) {
        const int tap = k / cin, ci = k - tap * cin, ky = tap / kw, kx = tap - ky * kw;
        v = w[(((size_t)n * cin + ci) * kh + ky) * kw + kx];
    }
    hi[t] = (uint16_t)bf16_bits(v);
    lo[t] = (uint16_t)bf16_bits(v - bf16_value(v));
}

namespace {

template <int NT, int PASSES>
int launch_nt(const char *name, const QConvArgs &q, bool vec)
{
    const dim3 grid(cdiv(q.a.M, Q_BM), q.a.npad / (32 * NT));
    if (vec)
        return launch(name, k_lfn_conv_q<NT, PASSES, true>, grid, dim3(Q_THREADS), 0, q);
    return launch(name, k_lfn_conv_q<NT, PASSES, false>, grid, dim3(Q_THREADS), 0, q);
}

} // namespace

int launch_conv_q(const char *name, const char *name_vec, const ConvArgs &a, const uint16_t *w_hi, const uint16_t *w_lo,
                  int kpad, int nt, int passes)
{
    QConvArgs q{a, w_hi, w_lo, kpad};
    const bool vec = a.cin % 4 == 0 && a.in_off % 4 == 0 && a.in_cs % 4 == 0 && (uintptr_t)a.in % 16 == 0;
    if (vec)
        name = name_vec;
    if (passes == 1) {
        switch (nt) {
        case 1: return launch_nt<1, 1>(name, q, vec);
        case 2: return launch_nt<2, 1>(name, q, vec);
        case 3: return launch_nt<3, 1>(name, q, vec);
        default: return launch_nt<4, 1>(name, q, vec);
        }
    }
    // bf16x3 stages two planes of each operand: at most 64 channels per block keep both buffers within 64 KB of LDS
    // (npad is a multiple of 32 nt: 128 -> 2 x 64, 96 -> 3 x 32)
    switch (nt) {
    case 2:
    case 4: return launch_nt<2, 3>(name, q, vec);
    default: return launch_nt<1, 3>(name, q, vec);
    }
}

int pack_weights_q(const Layer &l, const float *w, uint16_t *hi, uint16_t *lo)
{
    const size_t total = (size_t)l.npad * l.kpad;
    return launch("lfn_pack_q", k_lfn_pack_q, dim3(cdiv(total, 256)), dim3(256), 0, w, hi, lo, l.cout, l.cin, l.kh, l.kw,
                  l.npad, l.kpad);
}

} // namespace lfn
} // namespace tf
