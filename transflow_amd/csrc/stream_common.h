// What the byte-stream codecs (jpeg.hip, png.hip, flowzip.hip) share on the device: the prefix sum over a wave that
// places the lanes' bits, and the one-work-group exclusive sum that places the JPEG and PNG slots' bytes (flowzip.hip's
// scan folds the bands' CRCs between its barriers and has its own loop); and on the host the staging slots of the JPEG
// and PNG encoders with the protocol that takes their bytes to the caller (SlotStream).
#pragma once
#include <cstring>

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

// ---- the staging slots of the JPEG and PNG encoders, and how their bytes reach the caller.  The coding kernels fill a
// slot each and flag one that outgrows it, k_slot_scan places the slots, the encoder's pack kernel moves them to `packed`
// with `extra` bytes of its own around each (a JPEG interval's marker: 2, a PNG chunk's frame: 12), and the host copies
// head, packed stream and tail out.  An encode calls begin, its kernels, scan, its pack kernel with pack_room, fetch,
// the one hipStreamSynchronize, finish and copy_out; a copy_last calls have_last, the pack kernel and copy_out.
struct SlotStream {
    DevBuf staging, lengths, offsets, info, packed;
    PinnedBuf info_host; // page-locked unsigned long long: [0] the packed stream's bytes, [1] the overflow flag
    uint32_t slot = 0, extra = 0;
    int n = 0;
    size_t last = 0; // the packed stream's bytes of the last encode that ran; 0: none to copy again

    int alloc(int n_slots, uint32_t slot_bytes, uint32_t extra_bytes)
    {
        n = n_slots, slot = slot_bytes, extra = extra_bytes;
        const size_t count = (size_t)n;
        TF_TRY(staging.alloc(count * slot));
        TF_TRY(lengths.alloc(count * sizeof(uint32_t)));
        TF_TRY(offsets.alloc(count * sizeof(uint32_t)));
        TF_TRY(info.alloc(2 * sizeof(unsigned long long)));
        TF_TRY(packed.alloc(count * ((size_t)slot + extra))); // the worst case: every slot full
        return info_host.alloc(2 * sizeof(unsigned long long));
    }
    // nothing to copy again from here on, until finish() says that this encode's stream is whole
    int begin()
    {
        last = 0;
        TF_HIP(hipMemsetAsync(info.p, 0, info.bytes, stream()));
        return TF_OK;
    }
    uint32_t *overflow() const { return reinterpret_cast<uint32_t *>(info.as<unsigned long long>() + 1); } // what a coding kernel sets
    int scan(const char *label)
    {
        return launch(label, k_slot_scan, dim3(1), dim3(SCAN_BLOCK), 0, lengths.as<uint32_t>(), offsets.as<uint32_t>(), n, extra,
                      info.as<unsigned long long>());
    }
    // what the pack kernel may write: the caller's room behind a head of `head` bytes, and never more than the packed buffer
    size_t pack_room(size_t capacity, size_t head) const
    {
        const size_t room = capacity > head ? capacity - head : 0;
        return room < packed.bytes ? room : packed.bytes;
    }
    size_t pack_room() const { return packed.bytes; } // for a head that is not known before the kernels have run
    int fetch() // queued: the caller adds its own copies and waits once for all of them
    {
        TF_HIP(hipMemcpyAsync(info_host.p, info.p, info.bytes, hipMemcpyDeviceToHost, stream()));
        return TF_OK;
    }
    int finish(const char *who, const char *a_slot) // behind that wait
    {
        const unsigned long long *word = info_host.as<unsigned long long>();
        if (word[1])
            return set_error(TF_ERR_STATE, "%s: %s outgrew its staging slot of %u bytes", who, a_slot, slot);
        last = (size_t)word[0];
        return TF_OK;
    }
    int have_last(const char *who) const
    {
        return last ? TF_OK : set_error(TF_ERR_STATE, "%s: nothing has been encoded", who);
    }
    // head, packed stream and tail to the caller, if they fit; *n_bytes either way
    int copy_out(const char *who, const std::vector<uint8_t> &head, const std::vector<uint8_t> &tail, uint8_t *out, size_t capacity,
                 size_t *n_bytes) const
    {
        *n_bytes = head.size() + last + tail.size();
        TF_REQUIRE(*n_bytes <= capacity, "%s: the file has %zu bytes, the buffer %zu", who, *n_bytes, capacity);
        memcpy(out, head.data(), head.size());
        TF_HIP(hipMemcpyAsync(out + head.size(), packed.p, last, hipMemcpyDeviceToHost, stream()));
        TF_HIP(hipStreamSynchronize(stream()));
        if (!tail.empty())
            memcpy(out + head.size() + last, tail.data(), tail.size());
        return TF_OK;
    }
};

} // namespace tf
