// What the byte-stream codecs (jpeg.hip, png.hip, flowzip.hip) share on the device: the prefix sum over a wave that
// places the lanes' bits, and the one-work-group exclusive sum that places the JPEG and PNG slots' bytes (flowzip.hip's
// scan folds the bands' CRCs between its barriers and has its own loop).
#pragma once
#include "common.h"

namespace tf {

constexpr int WAVE = 64;

template <typename T> __device__ __forceinline__ T wave_inclusive_sum(T v, int lane)
{
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const T up = __shfl_up(v, d, WAVE);
        if (lane >= d)
            v += up;
    }
    return v;
}

// ---- the exclusive sum of any number of slots' byte counts by one work-group of SCAN_BLOCK threads, SCAN_BLOCK a trip
constexpr int SCAN_BLOCK = 1024;

// lengths[n] -> offsets[n], the exclusive sums of lengths[i] + extra (what is written around a slot's bytes: a PNG
// chunk's 12 bytes, a JPEG interval's marker); info[0] = their total.
// A trip has one barrier.  Every thread adds up all the waves' sums of the trip, so the carry from trip to trip is a
// register of each thread, and the waves' sums of two trips in turn have their own places in LDS: a wave that writes
// its sum of trip t + 2 has passed the barrier of trip t + 1, which every wave reaches with its loads of trip t done.
// (static: a unit that launches the kernel has its own, and a unit that does not has none.)
__attribute__((unused)) static __global__ __launch_bounds__(SCAN_BLOCK) void k_slot_scan(const uint32_t *__restrict__ lengths,
                                                                                         uint32_t *__restrict__ offsets, int n, uint32_t extra,
                                                                                         unsigned long long *__restrict__ info)
{
    constexpr int WAVES = SCAN_BLOCK / WAVE;
    __shared__ unsigned long long s_wave[2][WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    unsigned long long carry = 0;
    for (int base = 0, trip = 0; base < n; base += SCAN_BLOCK, trip++) {
        const int i = base + tid;
        const unsigned long long v = i < n ? (unsigned long long)lengths[i] + extra : 0;
        const unsigned long long incl = wave_inclusive_sum(v, lane);
        unsigned long long *sums = s_wave[trip & 1];
        if (lane == WAVE - 1)
            sums[wave] = incl;
        __syncthreads();
        unsigned long long before = carry;
#pragma unroll 4
        for (int w = 0; w < WAVES; w++) {
            const unsigned long long s = sums[w];
            carry += s;
            if (w < wave)
                before += s;
        }
        if (i < n)
            offsets[i] = (uint32_t)(before + incl - v);
    }
    if (tid == 0)
        info[0] = carry;
}

} // namespace tf
