// CRC-32 (reflected, polynomial EDB88320: zlib's, PNG's, zip's) as the device codecs compute it -- by slices: every lane
// takes a contiguous slice of the bytes through the byte table, a slice's CRC is moved in front of the bytes behind it
// by multiplying with x^(8 * bytes behind) modulo the polynomial, and the slices' CRCs are XORed.  A band's CRC is moved
// in front of the bands behind it the same way.  Host/device inline functions over plain memory: png.hip, flowzip.hip
// and flowunzip.hip run them on the device, tools/crc32_host_check.cpp on the CPU under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CRC_HD __host__ __device__ inline
#else
#define CRC_HD inline
#endif

namespace tf {

constexpr uint32_t CRC_POLY = 0xEDB88320u;

struct Crc32Consts {
    uint32_t crc[256]; // the byte table
    uint32_t x2n[32];  // x^(2^k) mod the polynomial (zlib's x2n_table)
};

// a(x) b(x) mod the polynomial, bit 31 the coefficient of x^0 (zlib's multmodp)
CRC_HD uint32_t multmodp(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0)
                break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8 n) mod the polynomial
CRC_HD uint32_t x8nmodp(uint32_t n, const uint32_t *x2n)
{
    uint32_t p = 1u << 31;
    for (int k = 3; n; n >>= 1, k++)
        if (n & 1)
            p = multmodp(x2n[k & 31], p);
    return p;
}

// the CRC-32 `c` of some bytes, moved in front of `bytes_behind` further bytes: XORed with the CRC-32 of those (and of
// whatever else the message has), it gives the whole message's.  (The CRC-32 of no bytes is 0 and stays 0.)
CRC_HD uint32_t crc32_shift(uint32_t c, uint32_t bytes_behind, const uint32_t *x2n)
{
    return (c && bytes_behind) ? multmodp(x8nmodp(bytes_behind, x2n), c) : c;
}

// the running register (a CRC-32's complement; all ones before the first byte) taken over one more byte
CRC_HD uint32_t crc32_update(uint32_t reg, uint32_t byte, const uint32_t *table)
{
    return table[(reg ^ byte) & 0xFF] ^ (reg >> 8);
}

CRC_HD void make_crc32_consts(Crc32Consts &c)
{
    for (uint32_t n = 0; n < 256; n++) {
        uint32_t v = n;
        for (int k = 0; k < 8; k++)
            v = (v & 1) ? (v >> 1) ^ CRC_POLY : v >> 1;
        c.crc[n] = v;
    }
    uint32_t p = 1u << 30; // x^1
    c.x2n[0] = p;
    for (int k = 1; k < 32; k++)
        c.x2n[k] = p = multmodp(p, p);
}

CRC_HD uint32_t crc32_bytes(const Crc32Consts &c, const uint8_t *p, size_t n)
{
    uint32_t reg = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++)
        reg = crc32_update(reg, p[i], c.crc);
    return ~reg;
}

#if defined(__HIPCC__)
// the tables into the caller's LDS arrays (256 and 32 words) by a work-group of `threads`; the caller sets the barrier
__device__ __forceinline__ void crc32_stage_table(uint32_t *s_crc, const Crc32Consts *__restrict__ c, int tid, int threads)
{
    for (int w = tid; w < 256; w += threads)
        s_crc[w] = c->crc[w];
}

__device__ __forceinline__ void crc32_stage_x2n(uint32_t *s_x2n, const Crc32Consts *__restrict__ c, int tid)
{
    if (tid < 32)
        s_x2n[tid] = c->x2n[tid];
}

// the XOR of the wave's 64 values, in every lane
__device__ __forceinline__ uint32_t crc32_wave_xor(uint32_t c)
{
#pragma unroll
    for (int d = 32; d; d >>= 1)
        c ^= __shfl_xor(c, d, 64);
    return c;
}
#endif

} // namespace tf
