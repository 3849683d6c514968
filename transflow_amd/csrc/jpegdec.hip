// Baseline JPEG decoded where the frame is wanted (tests/jpegdec_ref.py is the numpy statement of
// the same rules): libjpeg's pixels for SOF0 files of one interleaved scan, bit for bit -- jdhuff.c's decoding,
// jidctint.c's islow IDCT, jdsample.c's fancy upsampling, jdcolor.c's tables.  The header is walked on the host
// (jpegdec_common.h); the scan goes up as it is and the host looks at nothing behind SOS.
//
// Restart intervals are what make the entropy decoder parallel, as they do the encoder of jpeg.hip: DC prediction
// starts over and the stream is byte-aligned at each, and inside entropy-coded data an FF is always followed by 00, so
// every FF D0..D7 pair is a marker.
//
//   k_jd_count     every thread takes CHUNK bytes of the scan and counts the pairs FF D0..D7 that begin in them; a pair
//                  FF xx that is neither that nor FF 00 (nor the EOI the file ends with) rejects the file, and so does a
//                  scan that does not end with EOI.
//   k_slot_scan    the exclusive sum of the chunks' counts (one work-group; stream_common.h).
//   k_jd_markers   every thread walks its chunk again: marker k of the file, at the place the sum gives it, must be
//                  RST(k mod 8) and its position goes to markers[k]; the count must be ceil(MCUs / DRI) - 1.
//   k_jd_entropy   one wave per interval.  Lane 0 runs the machine of jpegdec_common.h over a window of the interval's
//                  bytes in LDS (the tables are in LDS too), block by block, into an MCU's dequantised coefficients in
//                  LDS; the wave refills the window with coalesced loads, zeroes the coefficients, and runs the column
//                  and the row pass of the IDCT, one lane per column or row of a block; a row's 8 samples go to the
//                  component's plane (padded to whole MCUs) as one 8-byte store.  A rejected interval leaves its
//                  number and reason in the status word (the lowest interval wins) and stops.
//   k_jd_colour    four adjacent pixels per lane: the chroma planes are upsampled (h2v2 / h2v1 fancy, with libjpeg's
//                  edge rules; replicated, as libjpeg does, where ceil(W / 2) <= 2), converted, and stored as three dwords.
//
// A file is untrusted.  Nothing it holds steers an address: intervals are clamped to the scan, the window to the
// interval, coefficient indices go through a table of 64 entries, and a plane store is placed by the MCU's number alone.
// Every kernel behind the marker scan returns at once when the status words already hold a rejection.
//
// A scan without restart markers is one interval, hence one wave, for k_jd_entropy.  tf_jpegdec_set_scan_mode(dec, 1)
// sends such a file down a second entropy path instead (jpegdec_par_common.h has its rules and the lane function):
//   k_jd_par_init   the scan minus the EOI is cut into subsequences of S bytes; each gets a guessed entry state.
//   k_jd_par_sync   one lane per subsequence, G per work-group: every lane decodes leniently from its entry, storing
//                   nothing, and hands its exit state to its neighbour, until no entry of the group changes (at most G
//                   rounds).  The group's exit goes to the next group's first entry; the host launches again while any
//                   of those changed (at most groups + 1 launches; a group whose first entry did not change does nothing).
//   k_slot_scan     four exclusive sums over the subsequences: the blocks that begin in each, the DC differences per component.
//   k_jd_par_write  one lane per subsequence decodes strictly from its now exact entry and stores undequantised int16
//                   coefficients at block * 64 + ZIGZAG[k]; the first fault (the lowest subsequence) is the verdict.
//   k_jd_par_idct   eight lanes per block: dequantise, column pass, row pass, the 8-byte stores of k_jd_entropy.
// A store is placed by a block number checked against the picture's block count, never by what the file says.
#include "jpegdec_common.h"
#include "jpegdec_par_common.h"
#include "stream_common.h"

#include <cstring>
#include <new>

namespace tf {
namespace jpegdec {

constexpr int CHUNK = 16;         // scan bytes per thread of the marker scan
constexpr int COUNT_BLOCK = 256;
constexpr uint32_t ST_NONE = 0xFFFFFFFFu;
constexpr int REASON_BITS = 5;    // status[1]: (interval << REASON_BITS) | reason
static_assert(R_COUNT <= (1 << REASON_BITS), "a reason must fit its bits");

struct Frame {
    const uint8_t *scan; // the bytes behind SOS, scan_bytes of them
    uint32_t scan_bytes;
    int W, H, components, h_samp, v_samp;
    int mcus_x, n_mcus, restart_mcus, intervals, blocks;
    int y_stride, c_stride; // the planes' row strides: mcus_x * 8 * h_samp, mcus_x * 8
    uint8_t *planes[3];
};

struct DevTables {
    Huff dc[3], ac[3];
    uint16_t quant[3][64];
};

// ---- the marker scan ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(COUNT_BLOCK) void k_jd_count(const uint8_t *__restrict__ scan, uint32_t n, uint32_t n_chunks,
                                                          uint32_t *__restrict__ counts, uint32_t *__restrict__ status)
{
    const uint32_t t = blockIdx.x * COUNT_BLOCK + threadIdx.x;
    if (t == 0 && (n < 2 || scan[n - 2] != 0xFF || scan[n - 1] != 0xD9))
        atomicMin(&status[0], (uint32_t)R_NO_EOI);
    if (t >= n_chunks)
        return;
    const uint32_t begin = t * CHUNK, end = min(begin + CHUNK, n); // (n_chunks * CHUNK < n + CHUNK <= 2^31 + CHUNK)
    uint32_t count = 0;
    bool stray = false;
    for (uint32_t i = begin; i < end; i++) {
        if (scan[i] != 0xFF)
            continue;
        if (i + 1 >= n) { // an FF the file ends with
            stray = true;
            continue;
        }
        const uint32_t kind = pair_kind(scan[i + 1]);
        count += kind == P_RST;
        stray |= kind == P_STRAY && !(i + 2 == n && scan[i + 1] == 0xD9);
    }
    counts[t] = count;
    if (stray)
        atomicMin(&status[0], (uint32_t)R_STRAY_MARKER);
}

__global__ __launch_bounds__(COUNT_BLOCK) void k_jd_markers(const uint8_t *__restrict__ scan, uint32_t n, uint32_t n_chunks,
                                                            const uint32_t *__restrict__ offsets, const unsigned long long *__restrict__ total,
                                                            uint32_t expected, uint32_t *__restrict__ markers, uint32_t *__restrict__ status)
{
    const uint32_t t = blockIdx.x * COUNT_BLOCK + threadIdx.x;
    if (t == 0 && total[0] != expected)
        atomicMin(&status[0], (uint32_t)R_RST_COUNT);
    if (t >= n_chunks)
        return;
    const uint32_t begin = t * CHUNK, end = min(begin + CHUNK, n);
    uint32_t k = offsets[t];
    bool order = false;
    for (uint32_t i = begin; i < end; i++) {
        if (scan[i] != 0xFF || i + 1 >= n || pair_kind(scan[i + 1]) != P_RST)
            continue;
        order |= scan[i + 1] != 0xD0 + (k & 7);
        if (k < expected) // markers[]: `expected` entries
            markers[k] = i;
        k++;
    }
    if (order)
        atomicMin(&status[0], (uint32_t)R_RST_ORDER);
}

// ---- entropy decoding and IDCT -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_jd_entropy(const Frame f, const DevTables *__restrict__ tables, const uint32_t *__restrict__ markers,
                                                     uint32_t *__restrict__ status, const FastDiv div_mcus_x)
{
    __shared__ DevTables s_t;
    __shared__ uint32_t s_win[WINDOW_BYTES / 4];
    __shared__ int32_t s_coef[MAX_BLOCKS][64];
    __shared__ int32_t s_ws[MAX_BLOCKS][64];
    const int lane = threadIdx.x;
    if (status[0] != ST_NONE) // the marker scan rejected the file: markers[] is not to be trusted
        return;
    const uint32_t iv = blockIdx.x;
    // the interval's bytes: from behind marker iv - 1 to marker iv; the last one ends at the EOI
    uint32_t from = iv == 0 ? 0 : markers[iv - 1] + 2;
    uint32_t to = iv + 1 == (uint32_t)f.intervals ? f.scan_bytes - 2 : markers[iv];
    to = min(to, f.scan_bytes), from = min(from, to); // (never: the marker scan wrote positions of the scan, in order)
    const uint8_t *src = f.scan + from;
    const uint32_t size = to - from;
    {
        const uint32_t *g = reinterpret_cast<const uint32_t *>(tables);
        uint32_t *s = reinterpret_cast<uint32_t *>(&s_t);
        for (uint32_t i = lane; i < sizeof(DevTables) / 4; i += WAVE)
            s[i] = g[i];
    }
    uint8_t *win = reinterpret_cast<uint8_t *>(s_win);
    Bits b;
    start(b, win, size);
    int last_dc[3] = {0, 0, 0};
    const int first = (int)iv * (f.restart_mcus ? f.restart_mcus : f.n_mcus); // (intervals * restart_mcus < n_mcus + 65536)
    const int last = min(first + (f.restart_mcus ? f.restart_mcus : f.n_mcus), f.n_mcus);
    const int luma_blocks = f.components == 1 ? 1 : f.h_samp * f.v_samp;
    __syncthreads();
    for (int m = first; m < last; m++) {
        for (int i = lane; i < f.blocks * 64; i += WAVE)
            (&s_coef[0][0])[i] = 0;
        for (int blk = 0; blk < f.blocks; blk++) {
            int need = lane == 0 ? (int)need_refill(b, BLOCK_MARGIN) : 0;
            need = __shfl(need, 0, WAVE);
            if (need) {
                uint32_t at = 0, len = 0;
                if (lane == 0)
                    refill_range(b, &at, &len);
                at = __shfl(at, 0, WAVE), len = __shfl(len, 0, WAVE);
                __syncthreads(); // lane 0 has read what it will of the old window
#pragma unroll
                for (uint32_t k = 0; k < WINDOW_BYTES / WAVE; k++) { // a fixed count: the loads go out together
                    const uint32_t i = k * WAVE + lane;
                    uint8_t v = 0;
                    if (i < len && at + i < size)
                        v = src[at + i];
                    if (i < len)
                        win[i] = v;
                }
            }
            __syncthreads(); // the window and the zeroed coefficients are in LDS
            uint32_t rc = R_OK;
            if (lane == 0) {
                const int c = blk < luma_blocks ? 0 : blk - luma_blocks + 1; // 0, 1, 2
                rc = decode_block(b, s_t.dc[c], s_t.ac[c], s_t.quant[c], last_dc[c], s_coef[blk]);
            }
            rc = __shfl(rc, 0, WAVE);
            if (rc != R_OK) {
                if (lane == 0)
                    atomicMin(&status[1], (iv << REASON_BITS) | rc);
                return;
            }
        }
        __syncthreads();
        const int blk = lane >> 3, sub = lane & 7;
        if (blk < f.blocks)
            idct_column(s_coef[blk], sub, s_ws[blk]);
        __syncthreads();
        if (blk < f.blocks) {
            uint8_t px[8];
            idct_row(s_ws[blk], sub, px);
            const int my = (int)fast_div((uint32_t)m, div_mcus_x), mx = m - my * f.mcus_x;
            uint8_t *dst;
            if (blk < luma_blocks) {
                const int by = blk / f.h_samp, bx = blk - by * f.h_samp; // (a grey file: h_samp 1)
                dst = f.planes[0] + ((size_t)(my * f.v_samp + by) * 8 + sub) * f.y_stride + (size_t)(mx * f.h_samp + bx) * 8;
            } else {
                dst = f.planes[blk - luma_blocks + 1] + ((size_t)my * 8 + sub) * f.c_stride + (size_t)mx * 8;
            }
            uint2 v;
            v.x = px[0] | (px[1] << 8) | (px[2] << 16) | ((uint32_t)px[3] << 24);
            v.y = px[4] | (px[5] << 8) | (px[6] << 16) | ((uint32_t)px[7] << 24);
            *reinterpret_cast<uint2 *>(dst) = v; // m < n_mcus: inside the plane of whole MCUs, 8-byte aligned
        }
        __syncthreads(); // s_coef and s_ws are read before the next MCU writes them
    }
}

// ---- the parallel path for a scan without restart markers -------------------------------------------------------------
constexpr int PAR_BLOCK = 256;         // threads of the init and write kernels
constexpr int PAR_MAX_GROUP = 256;     // G: subsequences (lanes) per work-group of the synchronisation
constexpr uint32_t PAR_DEFAULT_SUB = 64, PAR_DEFAULT_GROUP = 64; // measured: profiles/NOTES.md
constexpr int PAR_ENTRY_WORDS = 8;     // tf_jpegdec_par_entries: uint32 per subsequence

__device__ __forceinline__ void par_load_tables(DevTables &s_t, const DevTables *__restrict__ tables, int tid, int n_threads)
{
    const uint32_t *g = reinterpret_cast<const uint32_t *>(tables);
    uint32_t *s = reinterpret_cast<uint32_t *>(&s_t);
    for (uint32_t i = tid; i < sizeof(DevTables) / 4; i += n_threads)
        s[i] = g[i];
}

// first[0][] and first[1][]: the groups' first entries, read from one and written to the other launch by launch
__global__ __launch_bounds__(PAR_BLOCK) void k_jd_par_init(const uint8_t *__restrict__ scan, const ParGeom g, uint32_t group, uint64_t *__restrict__ entries,
                                                           uint64_t *__restrict__ first_a, uint64_t *__restrict__ first_b,
                                                           const uint32_t *__restrict__ status)
{
    if (status[0] != ST_NONE)
        return;
    const uint32_t i = blockIdx.x * PAR_BLOCK + threadIdx.x;
    if (i >= g.n_subs)
        return;
    const uint64_t e = i == 0 ? par_pack(0, 0, 0) : par_guess(scan, g.size, g.sub_bytes, i);
    entries[i] = e;
    if (i % group == 0)
        first_a[i / group] = first_b[i / group] = e;
}

// A work-group's share of the scan in LDS (option jd_par_staged; S a power of two): subsequence j of the group begins
// STAGE_PAD bytes behind where it would, so that lanes S bytes apart fall on different banks (at S = 128 they would all
// fall on one), and STAGE_TAIL bytes of the next group's share follow for the last lane's window.  What lies outside
// comes from memory.
constexpr uint32_t STAGE_PAD = 4, STAGE_TAIL = 16, STAGE_MAX_BYTES = 48 * 1024;
struct ParStaged {
    const uint8_t *scan, *lds;
    uint64_t first;   // the scan's byte lds[0] is
    uint32_t span;    // bytes of the scan that are in LDS
    uint32_t shift;   // log2 S
    __device__ __forceinline__ uint32_t at(uint64_t i) const
    {
        const uint64_t off = i - first; // (a lane reads from its entry on, at or behind its group's first byte)
        if (off < span)
            return lds[(uint32_t)off + (((uint32_t)off >> shift) * STAGE_PAD)];
        return scan[i];
    }
};

// info[0]: some group's first entry changed in this launch; info[1]: the largest round count of any group
template <bool STAGED>
__global__ __launch_bounds__(PAR_MAX_GROUP) void k_jd_par_sync(const uint8_t *__restrict__ scan, const ParGeom g, const DevTables *__restrict__ tables,
                                                               const uint32_t *__restrict__ status, uint64_t *__restrict__ entries,
                                                               uint32_t *__restrict__ n_begin, uint32_t *__restrict__ dc0, uint32_t *__restrict__ dc1,
                                                               uint32_t *__restrict__ dc2, const uint64_t *__restrict__ first_in,
                                                               uint64_t *__restrict__ first_out, uint64_t *__restrict__ seen, uint32_t *__restrict__ info,
                                                               int launch_no)
{
    __shared__ DevTables s_t;
    __shared__ uint64_t s_exit[PAR_MAX_GROUP];
    extern __shared__ uint32_t s_stage[]; // STAGED: group * (S + STAGE_PAD) + STAGE_TAIL bytes
    if (status[0] != ST_NONE)
        return;
    const uint32_t tid = threadIdx.x, group = blockDim.x, grp = blockIdx.x, n_groups = gridDim.x;
    const uint64_t e0 = first_in[grp];
    if (launch_no > 0 && seen[grp] == e0) { // what this group left the last time stands (uniform over the group)
        if (tid == 0 && grp + 1 < n_groups)
            first_out[grp + 1] = first_in[grp + 1];
        return;
    }
    par_load_tables(s_t, tables, (int)tid, (int)group);
    ParStaged staged;
    if (STAGED) {
        staged.scan = scan, staged.lds = reinterpret_cast<const uint8_t *>(s_stage);
        staged.first = (uint64_t)grp * group * g.sub_bytes; // a multiple of 4; below size: the group has a lane
        staged.shift = (uint32_t)__ffs((int)g.sub_bytes) - 1;
        const uint64_t left = g.size - staged.first;
        staged.span = (uint32_t)(left < (uint64_t)group * g.sub_bytes + STAGE_TAIL ? left : (uint64_t)group * g.sub_bytes + STAGE_TAIL);
        const uint32_t *words = reinterpret_cast<const uint32_t *>(scan + staged.first);
        // whole dwords: the last may reach into the EOI behind the data (the scan's buffer holds it), at() never reads it
        for (uint32_t d = tid; d < (staged.span + 3) / 4; d += group)
            s_stage[d + ((4 * d) >> staged.shift)] = words[d]; // (STAGE_PAD is one dword)
    }
    const uint32_t i = grp * group + tid;
    const bool active = i < g.n_subs;
    uint64_t entry = tid == 0 ? e0 : (active ? entries[i] : 0);
    bool changed = active;
    ParLane out;
    out.exit = 0, out.n_begin = 0, out.dc_sum[0] = out.dc_sum[1] = out.dc_sum[2] = 0, out.fault = 0;
    uint32_t rounds = 0;
    __syncthreads();
    for (uint32_t round = 0; round < group; round++) { // entry r of the group is exact after round r
        if (changed) {
            if (STAGED)
                par_lane<false>(staged, g, s_t.dc, s_t.ac, i, entry, 0u, nullptr, nullptr, out);
            else
                par_lane<false>(ParBytes{scan}, g, s_t.dc, s_t.ac, i, entry, 0u, nullptr, nullptr, out);
        }
        s_exit[tid] = out.exit;
        __syncthreads();
        const uint64_t handed = tid == 0 ? entry : s_exit[tid - 1];
        changed = active && handed != entry;
        entry = handed;
        rounds++;
        if (!__syncthreads_or((int)changed)) // (a barrier: s_exit is read before the next round writes it)
            break;
    }
    if (active) {
        entries[i] = entry;
        n_begin[i] = out.n_begin, dc0[i] = out.dc_sum[0], dc1[i] = out.dc_sum[1], dc2[i] = out.dc_sum[2];
    }
    if (tid == group - 1 && grp + 1 < n_groups) { // (active: only the last group has lanes behind the grid)
        first_out[grp + 1] = out.exit;
        if (out.exit != first_in[grp + 1])
            info[0] = 1;
    }
    if (tid == 0) {
        seen[grp] = e0;
        atomicMax(&info[1], rounds);
    }
}

__global__ __launch_bounds__(PAR_BLOCK) void k_jd_par_write(const uint8_t *__restrict__ scan, const ParGeom g, const DevTables *__restrict__ tables,
                                                            uint32_t *__restrict__ status, const uint64_t *__restrict__ entries,
                                                            const uint32_t *__restrict__ first_block, const uint32_t *__restrict__ pred0,
                                                            const uint32_t *__restrict__ pred1, const uint32_t *__restrict__ pred2,
                                                            const unsigned long long *__restrict__ total_begun, int16_t *__restrict__ coef)
{
    __shared__ DevTables s_t;
    if (status[0] != ST_NONE)
        return;
    par_load_tables(s_t, tables, (int)threadIdx.x, PAR_BLOCK);
    __syncthreads();
    const uint32_t i = blockIdx.x * PAR_BLOCK + threadIdx.x;
    if (i == 0 && total_begun[0] < g.total_blocks) // behind every lane's own fault
        atomicMin(&status[1], (g.n_subs << PAR_REASON_BITS) | (uint32_t)R_EXHAUSTED);
    if (i >= g.n_subs)
        return;
    const uint32_t pred[3] = {pred0[i], pred1[i], pred2[i]};
    ParLane out;
    par_lane<true>(ParBytes{scan}, g, s_t.dc, s_t.ac, i, entries[i], first_block[i], pred, coef, out);
    if (out.fault != R_OK)
        atomicMin(&status[1], (i << PAR_REASON_BITS) | out.fault);
}

// tf_jpegdec_par_entries' rows
__global__ __launch_bounds__(PAR_BLOCK) void k_jd_par_entries(uint32_t n_subs, const uint64_t *__restrict__ entries, const uint32_t *__restrict__ first_block,
                                                              const uint32_t *__restrict__ pred0, const uint32_t *__restrict__ pred1,
                                                              const uint32_t *__restrict__ pred2, uint32_t *__restrict__ rows)
{
    const uint32_t i = blockIdx.x * PAR_BLOCK + threadIdx.x;
    if (i >= n_subs)
        return;
    const uint64_t e = entries[i];
    uint32_t *r = rows + (size_t)i * PAR_ENTRY_WORDS;
    r[0] = (uint32_t)par_pos(e), r[1] = (uint32_t)(par_pos(e) >> 32), r[2] = par_blk(e), r[3] = par_k(e);
    r[4] = first_block[i], r[5] = pred0[i], r[6] = pred1[i], r[7] = pred2[i];
}

constexpr int IDCT_BLOCK = 256, IDCT_BLOCKS = IDCT_BLOCK / 8; // 8 lanes a block
constexpr int IDCT_STRIDE = 72; // dwords between two blocks in LDS: the column pass's lanes (block, column) fall on 64 different banks
__global__ __launch_bounds__(IDCT_BLOCK) void k_jd_par_idct(const Frame f, const DevTables *__restrict__ tables, const int16_t *__restrict__ coef,
                                                            uint32_t total_blocks, const uint32_t *__restrict__ status, const FastDiv div_mcus_x,
                                                            const FastDiv div_blocks)
{
    __shared__ uint16_t s_q[3][64]; // by natural position
    __shared__ int32_t s_coef[IDCT_BLOCKS][IDCT_STRIDE];
    __shared__ int32_t s_ws[IDCT_BLOCKS][IDCT_STRIDE];
    if (status[0] != ST_NONE || status[1] != ST_NONE)
        return;
    const int tid = threadIdx.x;
    if (tid < 192)
        s_q[tid >> 6][ZIGZAG[tid & 63]] = tables->quant[tid >> 6][tid & 63];
    __syncthreads();
    const int local = tid >> 3, sub = tid & 7;
    const uint32_t j = blockIdx.x * IDCT_BLOCKS + local;
    const bool valid = j < total_blocks;
    const int luma_blocks = f.components == 1 ? 1 : f.h_samp * f.v_samp;
    const int m = (int)fast_div(valid ? j : 0u, div_blocks), blk = (int)(valid ? j : 0u) - m * f.blocks;
    const int c = blk < luma_blocks ? 0 : blk - luma_blocks + 1;
    if (valid) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(coef + (size_t)j * 64 + sub * 8); // row `sub`: 16 bytes, aligned
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int x = 0; x < 8; x++) {
            const int32_t v = (int16_t)(w[x >> 1] >> (16 * (x & 1)));
            s_coef[local][sub * 8 + x] = v * (int32_t)s_q[c][sub * 8 + x];
        }
    }
    __syncthreads();
    if (valid)
        idct_column(s_coef[local], sub, s_ws[local]);
    __syncthreads();
    if (valid) {
        uint8_t px[8];
        idct_row(s_ws[local], sub, px);
        const int my = (int)fast_div((uint32_t)m, div_mcus_x), mx = m - my * f.mcus_x;
        uint8_t *dst;
        if (blk < luma_blocks) {
            const int by = blk / f.h_samp, bx = blk - by * f.h_samp;
            dst = f.planes[0] + ((size_t)(my * f.v_samp + by) * 8 + sub) * f.y_stride + (size_t)(mx * f.h_samp + bx) * 8;
        } else {
            dst = f.planes[blk - luma_blocks + 1] + ((size_t)my * 8 + sub) * f.c_stride + (size_t)mx * 8;
        }
        uint2 v;
        v.x = px[0] | (px[1] << 8) | (px[2] << 16) | ((uint32_t)px[3] << 24);
        v.y = px[4] | (px[5] << 8) | (px[6] << 16) | ((uint32_t)px[7] << 24);
        *reinterpret_cast<uint2 *>(dst) = v; // j < total_blocks, so m < n_mcus: inside the plane of whole MCUs, 8-byte aligned
    }
}

// ---- upsampling and colour -------------------------------------------------------------------------------------------------
// jdsample.c h2v1_fancy_upsample at output column x of a row whose `dw` samples begin at p
__device__ __forceinline__ int up_h2v1(const uint8_t *p, int dw, int x)
{
    const int c = x >> 1;
    if (c == 0)
        return (x & 1) ? (p[0] * 3 + p[1] + 2) >> 2 : p[0]; // (p[1] exists: a plane row has at least 8 samples)
    if (c == dw - 1)
        return (x & 1) ? p[c] : (p[c] * 3 + p[c - 1] + 1) >> 2;
    return (x & 1) ? (p[c] * 3 + p[c + 1] + 2) >> 2 : (p[c] * 3 + p[c - 1] + 1) >> 2;
}

// jdsample.c h2v2_fancy_upsample: p0 the chroma row the output row lies in, p1 the nearer of its neighbours
__device__ __forceinline__ int up_h2v2(const uint8_t *p0, const uint8_t *p1, int dw, int x)
{
    const int c = x >> 1;
    const int cur = p0[c] * 3 + p1[c];
    if (c == 0)
        return (x & 1) ? (cur * 3 + (p0[1] * 3 + p1[1]) + 7) >> 4 : (cur * 4 + 8) >> 4;
    if (c == dw - 1)
        return (x & 1) ? (cur * 4 + 7) >> 4 : (cur * 3 + (p0[c - 1] * 3 + p1[c - 1]) + 8) >> 4;
    return (x & 1) ? (cur * 3 + (p0[c + 1] * 3 + p1[c + 1]) + 7) >> 4 : (cur * 3 + (p0[c - 1] * 3 + p1[c - 1]) + 8) >> 4;
}

__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

constexpr int COLOUR_BLOCK = 256;
constexpr int PX_PER_LANE = 4;
__global__ __launch_bounds__(COLOUR_BLOCK) void k_jd_colour(const Frame f, uint8_t *__restrict__ out, int bgr, int aligned,
                                                            const uint32_t *__restrict__ status, const FastDiv div_w)
{
    if (status[0] != ST_NONE || status[1] != ST_NONE)
        return;
    const uint32_t n_px = (uint32_t)f.W * (uint32_t)f.H; // (the handle's limit: below 2^28)
    const uint32_t p0 = (blockIdx.x * COLOUR_BLOCK + threadIdx.x) * PX_PER_LANE;
    if (p0 >= n_px)
        return;
    const int dw = (f.W + 1) / 2, dh = (f.H + 1) / 2; // the chroma planes' real samples (h_samp 2, v_samp 2)
    uint8_t bytes[3 * PX_PER_LANE];
#pragma unroll
    for (int k = 0; k < PX_PER_LANE; k++) {
        const uint32_t p = min(p0 + k, n_px - 1);
        const int y = (int)fast_div(p, div_w), x = (int)(p - (uint32_t)y * f.W);
        const int Y = f.planes[0][(size_t)y * f.y_stride + x];
        int r = Y, g = Y, b = Y;
        if (f.components == 3) {
            int cb, cr;
            if (f.h_samp == 1) {
                cb = f.planes[1][(size_t)y * f.c_stride + x], cr = f.planes[2][(size_t)y * f.c_stride + x];
            } else if (dw <= 2) { // jinit_upsampler: h2v1_upsample / h2v2_upsample, the sample replicated, for W <= 4
                const size_t at = (size_t)(y >> (f.v_samp - 1)) * f.c_stride + (x >> 1);
                cb = f.planes[1][at], cr = f.planes[2][at];
            } else if (f.v_samp == 1) {
                cb = up_h2v1(f.planes[1] + (size_t)y * f.c_stride, dw, x);
                cr = up_h2v1(f.planes[2] + (size_t)y * f.c_stride, dw, x);
            } else {
                const int row = y >> 1;
                const int other = (y & 1) ? min(row + 1, dh - 1) : max(row - 1, 0); // jdmainct.c: the edge rows repeat
                cb = up_h2v2(f.planes[1] + (size_t)row * f.c_stride, f.planes[1] + (size_t)other * f.c_stride, dw, x);
                cr = up_h2v2(f.planes[2] + (size_t)row * f.c_stride, f.planes[2] + (size_t)other * f.c_stride, dw, x);
            }
            // jdcolor.c build_ycc_rgb_table, SCALEBITS 16
            cb -= 128, cr -= 128;
            r = (int)clamp255(Y + ((91881 * cr + 32768) >> 16));
            g = (int)clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
            b = (int)clamp255(Y + ((116130 * cb + 32768) >> 16));
        }
        bytes[3 * k] = (uint8_t)(bgr ? b : r), bytes[3 * k + 1] = (uint8_t)g, bytes[3 * k + 2] = (uint8_t)(bgr ? r : b);
    }
    uint8_t *dst = out + (size_t)p0 * 3;
    if (aligned && p0 + PX_PER_LANE <= n_px) {
        uint32_t *d = reinterpret_cast<uint32_t *>(dst);
#pragma unroll
        for (int w = 0; w < 3; w++)
            d[w] = bytes[4 * w] | (bytes[4 * w + 1] << 8) | (bytes[4 * w + 2] << 16) | ((uint32_t)bytes[4 * w + 3] << 24);
    } else {
        const uint32_t n = min((uint32_t)PX_PER_LANE, n_px - p0) * 3;
        for (uint32_t i = 0; i < n; i++)
            dst[i] = bytes[i];
    }
}

} // namespace jpegdec
} // namespace tf

using namespace tf;
using namespace tf::jpegdec;

struct tf_jpegdec {
    int max_w = 0, max_h = 0;
    size_t max_file = 0, max_chunks = 0, max_intervals = 0, plane_room = 0;
    DevBuf tables, scan, counts, offsets, total, markers, status, planes, out;
    PinnedBuf stage;       // page-locked uint8_t: the scan's bytes on their way up
    PinnedBuf tables_host; // page-locked DevTables
    PinnedBuf status_host; // page-locked uint32_t: the two status words
    Header header;
    Raw raw;
    // the parallel path for scans without restart markers: allocated by the first decode that takes it
    int scan_mode = 0;
    size_t max_subs = 0, max_groups = 0, max_blocks = 0;
    DevBuf par_entries, par_counts, par_offsets, par_first, par_totals, par_info, par_coef, par_rows;
    PinnedBuf par_info_host; // page-locked uint32_t: the two info words
    uint32_t par_stats[4] = {0, 0, 0, 0};
    uint32_t par_last_subs = 0; // the subsequences of the last decode that took the path (0: none has)
};

static int par_ensure(tf_jpegdec *dec)
{
    if (dec->par_coef.p)
        return TF_OK;
    const size_t subs = dec->max_subs, groups = dec->max_groups;
    TF_TRY(dec->par_entries.alloc(subs * sizeof(uint64_t)));
    TF_TRY(dec->par_counts.alloc(4 * subs * sizeof(uint32_t)));
    TF_TRY(dec->par_offsets.alloc(4 * subs * sizeof(uint32_t)));
    TF_TRY(dec->par_first.alloc(3 * groups * sizeof(uint64_t)));
    TF_TRY(dec->par_totals.alloc(4 * sizeof(unsigned long long)));
    TF_TRY(dec->par_info.alloc(2 * sizeof(uint32_t)));
    TF_TRY(dec->par_info_host.alloc(2 * sizeof(uint32_t)));
    TF_TRY(dec->par_coef.alloc(dec->max_blocks * 64 * sizeof(int16_t)));
    return TF_OK;
}

// the entropy stage of a scan without restart markers; the marker scan is queued, the colour kernel follows
static int par_decode(tf_jpegdec *dec, const Frame &f, uint32_t *status)
{
    const long opt_sub = option(OPT_JD_PAR_SUB_BYTES), opt_group = option(OPT_JD_PAR_GROUP_SUBS), opt_staged = option(OPT_JD_PAR_STAGED);
    TF_REQUIRE(opt_sub == 0 || (opt_sub >= (long)PAR_MIN_SUB && opt_sub <= (long)PAR_MAX_SUB), "jd_par_sub_bytes: %ld (0, or %u to %u)", opt_sub,
               PAR_MIN_SUB, PAR_MAX_SUB);
    TF_REQUIRE(opt_group == 0 || opt_group == 64 || opt_group == 128 || opt_group == 256, "jd_par_group_subs: %ld (0, 64, 128 or 256)", opt_group);
    TF_TRY(par_ensure(dec));
    ParGeom g;
    g.size = f.scan_bytes - 2;
    g.sub_bytes = opt_sub ? (uint32_t)opt_sub : PAR_DEFAULT_SUB;
    g.n_subs = par_subs(g.size, g.sub_bytes);
    g.blocks = (uint32_t)f.blocks, g.luma_blocks = f.components == 1 ? 1u : (uint32_t)(f.h_samp * f.v_samp);
    g.total_blocks = (uint32_t)f.n_mcus * (uint32_t)f.blocks;
    const uint32_t group = opt_group ? (uint32_t)opt_group : PAR_DEFAULT_GROUP;
    const uint32_t n_groups = cdiv(g.n_subs, group);
    TF_REQUIRE(g.n_subs <= dec->max_subs && n_groups <= dec->max_groups && g.total_blocks <= dec->max_blocks,
               "tf_jpegdec_decode_dev: %u subsequences, %u blocks: beyond the handle", g.n_subs, g.total_blocks);
    const size_t subs = dec->max_subs;
    uint64_t *entries = dec->par_entries.as<uint64_t>();
    uint32_t *counts = dec->par_counts.as<uint32_t>(), *offsets = dec->par_offsets.as<uint32_t>();
    uint64_t *first[2] = {dec->par_first.as<uint64_t>(), dec->par_first.as<uint64_t>() + dec->max_groups};
    uint64_t *seen = dec->par_first.as<uint64_t>() + 2 * dec->max_groups;
    uint32_t *info = dec->par_info.as<uint32_t>();
    unsigned long long *totals = dec->par_totals.as<unsigned long long>();
    const DevTables *tables = dec->tables.as<DevTables>();
    TF_HIP(hipMemsetAsync(dec->par_coef.p, 0, (size_t)g.total_blocks * 64 * sizeof(int16_t), stream()));
    TF_HIP(hipMemsetAsync(info, 0, 2 * sizeof(uint32_t), stream()));
    TF_TRY(launch("jd_par_init", k_jd_par_init, dim3(cdiv(g.n_subs, PAR_BLOCK)), dim3(PAR_BLOCK), 0, f.scan, g, group, entries, first[0], first[1],
                  (const uint32_t *)status));
    // the group's share in LDS: where S is a power of two and the share fits
    const size_t stage_bytes = ((size_t)group * (g.sub_bytes + STAGE_PAD) + STAGE_TAIL + 3) / 4 * 4;
    const bool staged = opt_staged == 1 && (g.sub_bytes & (g.sub_bytes - 1)) == 0 && stage_bytes <= STAGE_MAX_BYTES;
    uint32_t launches = 0;
    const uint32_t *info_host = dec->par_info_host.as<uint32_t>();
    for (uint32_t l = 0; l <= n_groups; l++) { // entry r of the file is exact after launch r: at most n_groups + 1
        if (l)
            TF_HIP(hipMemsetAsync(info, 0, sizeof(uint32_t), stream()));
        if (staged)
            TF_TRY(launch("jd_par_sync", k_jd_par_sync<true>, dim3(n_groups), dim3(group), stage_bytes, f.scan, g, tables, (const uint32_t *)status,
                          entries, counts, counts + subs, counts + 2 * subs, counts + 3 * subs, (const uint64_t *)first[l & 1], first[(l & 1) ^ 1],
                          seen, info, (int)l));
        else
            TF_TRY(launch("jd_par_sync", k_jd_par_sync<false>, dim3(n_groups), dim3(group), 0, f.scan, g, tables, (const uint32_t *)status,
                          entries, counts, counts + subs, counts + 2 * subs, counts + 3 * subs, (const uint64_t *)first[l & 1], first[(l & 1) ^ 1],
                          seen, info, (int)l));
        launches++;
        TF_HIP(hipMemcpyAsync(dec->par_info_host.p, info, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
        TF_HIP(hipStreamSynchronize(stream()));
        if (!info_host[0])
            break;
    }
    for (int a = 0; a < 4; a++)
        TF_TRY(launch("jd_par_scan", k_slot_scan, dim3(1), dim3(SCAN_BLOCK), 0, (const uint32_t *)(counts + a * subs), offsets + a * subs, (int)g.n_subs,
                      0u, totals + a));
    TF_TRY(launch("jd_par_write", k_jd_par_write, dim3(cdiv(g.n_subs, PAR_BLOCK)), dim3(PAR_BLOCK), 0, f.scan, g, tables, status,
                  (const uint64_t *)entries, (const uint32_t *)offsets, (const uint32_t *)(offsets + subs), (const uint32_t *)(offsets + 2 * subs),
                  (const uint32_t *)(offsets + 3 * subs), (const unsigned long long *)totals, dec->par_coef.as<int16_t>()));
    TF_TRY(launch("jd_par_idct", k_jd_par_idct, dim3(cdiv(g.total_blocks, IDCT_BLOCKS)), dim3(IDCT_BLOCK), 0, f, tables,
                  (const int16_t *)dec->par_coef.as<int16_t>(), g.total_blocks, (const uint32_t *)status, fast_div_setup((uint32_t)f.mcus_x),
                  fast_div_setup((uint32_t)f.blocks)));
    dec->par_stats[0] = g.n_subs, dec->par_stats[1] = n_groups, dec->par_stats[2] = launches, dec->par_stats[3] = info_host[1];
    dec->par_last_subs = g.n_subs;
    return TF_OK;
}

TF_API int tf_jpegdec_set_scan_mode(tf_jpegdec *dec, int mode)
{
    TF_REQUIRE(dec, "tf_jpegdec_set_scan_mode: null pointer");
    TF_REQUIRE(mode == 0 || mode == 1, "tf_jpegdec_set_scan_mode: mode %d (0 one wave per restart interval, 1 scans without DRI in parallel)", mode);
    dec->scan_mode = mode;
    return TF_OK;
}

TF_API int tf_jpegdec_par_stats(tf_jpegdec *dec, uint32_t out[4])
{
    TF_REQUIRE(dec && out, "tf_jpegdec_par_stats: null pointer");
    memcpy(out, dec->par_stats, sizeof(dec->par_stats));
    return TF_OK;
}

TF_API int tf_jpegdec_par_entries(tf_jpegdec *dec, uint32_t *rows, size_t capacity, uint32_t *n_subs)
{
    TF_REQUIRE(dec && rows && n_subs, "tf_jpegdec_par_entries: null pointer");
    const uint32_t n = dec->par_last_subs;
    *n_subs = n;
    TF_REQUIRE(n > 0, "tf_jpegdec_par_entries: no decode of this handle has taken the parallel path");
    TF_REQUIRE(capacity >= n, "tf_jpegdec_par_entries: room for %zu subsequences, the last decode had %u", capacity, n);
    const size_t bytes = (size_t)n * PAR_ENTRY_WORDS * sizeof(uint32_t), subs = dec->max_subs;
    if (dec->par_rows.bytes < bytes)
        TF_TRY(dec->par_rows.alloc(bytes));
    const uint32_t *offsets = dec->par_offsets.as<uint32_t>();
    TF_TRY(launch("jd_par_entries", k_jd_par_entries, dim3(cdiv(n, PAR_BLOCK)), dim3(PAR_BLOCK), 0, n, (const uint64_t *)dec->par_entries.as<uint64_t>(),
                  offsets, offsets + subs, offsets + 2 * subs, offsets + 3 * subs, dec->par_rows.as<uint32_t>()));
    TF_HIP(hipMemcpyAsync(rows, dec->par_rows.p, bytes, hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    return TF_OK;
}

TF_API const char *tf_jpegdec_reject_name(uint32_t reject) { return reject_name(reject); }

TF_API int tf_jpegdec_probe(const uint8_t *file, size_t n, tf_jpegdec_info *info)
{
    TF_REQUIRE((file || n == 0) && info, "tf_jpegdec_probe: null pointer");
    static thread_local Header hd; // 20 KB with `raw`: the walker's working space, one per calling thread
    static thread_local Raw raw;
    const uint32_t r = parse_header(file, n, hd, raw);
    memset(info, 0, sizeof(*info));
    info->reject = r;
    if (r == R_OK) {
        info->width = hd.width, info->height = hd.height, info->components = hd.components;
        info->h_samp = hd.h_samp, info->v_samp = hd.v_samp, info->restart_mcus = hd.restart_mcus, info->intervals = hd.intervals;
    }
    return TF_OK;
}

TF_API void tf_jpegdec_destroy(tf_jpegdec *dec) { delete dec; }

TF_API int tf_jpegdec_create(tf_jpegdec **out, int max_width, int max_height, size_t max_file_bytes)
{
    TF_REQUIRE(out, "tf_jpegdec_create: null pointer");
    *out = nullptr;
    TF_REQUIRE(max_width >= 1 && max_height >= 1 && max_width <= 16384 && max_height <= 16384, "tf_jpegdec_create: bad size %dx%d (1 to 16384)",
               max_width, max_height);
    TF_REQUIRE(max_file_bytes >= 1 && max_file_bytes <= ((size_t)1 << 30), "tf_jpegdec_create: a file of %zu bytes (1 to 2^30)", max_file_bytes);
    TF_TRY(ensure_init());
    auto dec = make_handle<tf_jpegdec>();
    TF_REQUIRE(dec, "tf_jpegdec_create: out of memory");
    dec->max_w = max_width, dec->max_h = max_height, dec->max_file = max_file_bytes;
    dec->max_chunks = (max_file_bytes + CHUNK - 1) / CHUNK;
    // the MCUs of the smallest MCU (8 x 8) bound the intervals; a plane of whole 16 x 16 MCUs bounds every sampling's
    const size_t pw = ((size_t)max_width + 15) / 16 * 16, ph = ((size_t)max_height + 15) / 16 * 16;
    dec->max_intervals = (pw / 8) * (ph / 8);
    dec->plane_room = pw * ph;
    // the parallel path's buffers (allocated when it is first taken): the smallest subsequence and group bound their
    // counts, three components at 1 x 1 the blocks
    dec->max_subs = (max_file_bytes + PAR_MIN_SUB - 1) / PAR_MIN_SUB;
    dec->max_groups = (dec->max_subs + 63) / 64;
    dec->max_blocks = 3 * dec->max_intervals;
    TF_TRY(dec->tables.alloc(sizeof(DevTables)));
    TF_TRY(dec->scan.alloc(max_file_bytes + 4));
    TF_TRY(dec->counts.alloc(dec->max_chunks * sizeof(uint32_t)));
    TF_TRY(dec->offsets.alloc(dec->max_chunks * sizeof(uint32_t)));
    TF_TRY(dec->total.alloc(sizeof(unsigned long long)));
    TF_TRY(dec->markers.alloc(dec->max_intervals * sizeof(uint32_t)));
    TF_TRY(dec->status.alloc(2 * sizeof(uint32_t)));
    TF_TRY(dec->planes.alloc(3 * dec->plane_room));
    TF_TRY(dec->stage.alloc(max_file_bytes));
    TF_TRY(dec->tables_host.alloc(sizeof(DevTables)));
    TF_TRY(dec->status_host.alloc(2 * sizeof(uint32_t)));
    *out = dec.release();
    return TF_OK;
}

TF_API int tf_jpegdec_decode_dev(tf_jpegdec *dec, const uint8_t *file, size_t n, void *out_dev, int order, uint32_t *reject)
{
    TF_REQUIRE(dec && (file || n == 0) && out_dev && reject, "tf_jpegdec_decode_dev: null pointer");
    TF_REQUIRE(order == 0 || order == 1, "tf_jpegdec_decode_dev: order %d (0 RGB, 1 BGR)", order);
    *reject = R_OK;
    Header &hd = dec->header;
    const uint32_t r = parse_header(file, n, hd, dec->raw);
    if (r != R_OK) {
        *reject = r;
        return TF_OK;
    }
    TF_REQUIRE(hd.width <= dec->max_w && hd.height <= dec->max_h, "tf_jpegdec_decode_dev: a frame of %dx%d, the handle is for %dx%d", hd.width,
               hd.height, dec->max_w, dec->max_h);
    const size_t scan_bytes = n - hd.scan_offset;
    TF_REQUIRE(scan_bytes <= dec->max_file, "tf_jpegdec_decode_dev: a scan of %zu bytes, the handle is for %zu", scan_bytes, dec->max_file);
    if (scan_bytes < 2) { // not even an EOI; nothing to send
        *reject = R_NO_EOI;
        return TF_OK;
    }
    Frame f;
    f.scan = dec->scan.as<uint8_t>(), f.scan_bytes = (uint32_t)scan_bytes;
    f.W = hd.width, f.H = hd.height, f.components = hd.components, f.h_samp = hd.h_samp, f.v_samp = hd.v_samp;
    f.mcus_x = hd.mcus_x, f.n_mcus = hd.n_mcus, f.restart_mcus = hd.restart_mcus, f.intervals = hd.intervals, f.blocks = hd.blocks_per_mcu;
    f.y_stride = hd.mcus_x * 8 * hd.h_samp, f.c_stride = hd.mcus_x * 8;
    // (the planes of whole MCUs fit: an MCU is at most 16 x 16 and the frame at most the handle's size)
    const size_t y_bytes = (size_t)f.y_stride * hd.mcus_y * 8 * hd.v_samp, c_bytes = (size_t)f.c_stride * hd.mcus_y * 8;
    TF_REQUIRE(y_bytes <= dec->plane_room && c_bytes <= dec->plane_room && (size_t)hd.intervals <= dec->max_intervals,
               "tf_jpegdec_decode_dev: planes of %zu bytes, %d intervals: beyond the handle", y_bytes, hd.intervals);
    for (int c = 0; c < 3; c++)
        f.planes[c] = dec->planes.as<uint8_t>() + (size_t)c * dec->plane_room;
    DevTables &t = *dec->tables_host.as<DevTables>();
    for (int c = 0; c < 3; c++) {
        const int s = c < hd.components ? c : 0;
        t.dc[c] = hd.dc[s], t.ac[c] = hd.ac[s];
        memcpy(t.quant[c], hd.quant[s], sizeof(t.quant[c]));
    }
    memcpy(dec->stage.p, file + hd.scan_offset, scan_bytes);
    const uint32_t n_chunks = (uint32_t)((scan_bytes + CHUNK - 1) / CHUNK);
    const uint32_t expected = (uint32_t)hd.intervals - 1;
    uint32_t *status = dec->status.as<uint32_t>();
    TF_HIP(hipMemcpyAsync(dec->scan.p, dec->stage.p, scan_bytes, hipMemcpyHostToDevice, stream()));
    TF_HIP(hipMemcpyAsync(dec->tables.p, dec->tables_host.p, sizeof(DevTables), hipMemcpyHostToDevice, stream()));
    TF_HIP(hipMemsetAsync(dec->status.p, 0xFF, 2 * sizeof(uint32_t), stream()));
    TF_TRY(launch("jd_count", k_jd_count, dim3(cdiv(n_chunks, COUNT_BLOCK)), dim3(COUNT_BLOCK), 0, f.scan, f.scan_bytes, n_chunks,
                  dec->counts.as<uint32_t>(), status));
    TF_TRY(launch("jd_scan", k_slot_scan, dim3(1), dim3(SCAN_BLOCK), 0, dec->counts.as<uint32_t>(), dec->offsets.as<uint32_t>(), (int)n_chunks, 0u,
                  dec->total.as<unsigned long long>()));
    TF_TRY(launch("jd_markers", k_jd_markers, dim3(cdiv(n_chunks, COUNT_BLOCK)), dim3(COUNT_BLOCK), 0, f.scan, f.scan_bytes, n_chunks,
                  dec->offsets.as<uint32_t>(), dec->total.as<unsigned long long>(), expected, dec->markers.as<uint32_t>(), status));
    if (dec->scan_mode == 1 && hd.restart_mcus == 0)
        TF_TRY(par_decode(dec, f, status));
    else
        TF_TRY(launch("jd_entropy", k_jd_entropy, dim3((unsigned)hd.intervals), dim3(WAVE), 0, f, dec->tables.as<DevTables>(),
                      dec->markers.as<uint32_t>(), status, fast_div_setup((uint32_t)hd.mcus_x)));
    const size_t n_px = (size_t)hd.width * hd.height;
    TF_TRY(launch("jd_colour", k_jd_colour, dim3(cdiv(n_px, (size_t)COLOUR_BLOCK * PX_PER_LANE)), dim3(COLOUR_BLOCK), 0, f, (uint8_t *)out_dev, order,
                  (int)((uintptr_t)out_dev % 4 == 0), status, fast_div_setup((uint32_t)hd.width)));
    TF_HIP(hipMemcpyAsync(dec->status_host.p, dec->status.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
    TF_HIP(hipStreamSynchronize(stream()));
    const uint32_t *st = dec->status_host.as<uint32_t>();
    if (st[0] != ST_NONE)
        *reject = st[0];
    else if (st[1] != ST_NONE)
        *reject = st[1] & ((1u << REASON_BITS) - 1);
    return TF_OK;
}

TF_API int tf_jpegdec_decode(tf_jpegdec *dec, const uint8_t *file, size_t n, uint8_t *out_host, int order, uint32_t *reject)
{
    TF_REQUIRE(dec && out_host && reject, "tf_jpegdec_decode: null pointer");
    if (!dec->out.p)
        TF_TRY(dec->out.alloc((size_t)dec->max_w * dec->max_h * 3 + 4));
    TF_TRY(tf_jpegdec_decode_dev(dec, file, n, dec->out.p, order, reject));
    if (*reject == R_OK) {
        TF_HIP(hipMemcpyAsync(out_host, dec->out.p, (size_t)dec->header.width * dec->header.height * 3, hipMemcpyDeviceToHost, stream()));
        TF_HIP(hipStreamSynchronize(stream()));
    }
    return TF_OK;
}
