// numpy's legacy random stream (MT19937, RandomState.random_sample) drawn on the device, bit for bit: fields of n
// doubles = N = 2 n stream words, for the compositor's random reset (reference.py:59).  DESIGN.md section 24.
//
//   k_mt_fill   one wave per segment of S words: the 624-word window in a 1024-word LDS ring, 226 new words a step,
//               tempered, paired into doubles and stored coalesced; the segment's first PREFIX raw words go to a
//               scratch for the jump
//   k_mt_jump   segment g's start state for the NEXT field: Y[g][j] = XOR over the set coefficients i of t^N mod phi
//               of X[g][i + j] -- the same polynomial for every segment; a block takes a quarter of the exponents and
//               stages the words they reach in LDS, the fill XORs the four partial states when it loads them
//   k_mt_walk   the bootstrap after a state is adopted or the field size changes: one wave walks the first field's span
//               and leaves the window at every segment start
//   k_mt_combine  the state at the stream's position (segment 0's start state), for tf_mt_get_state and a size change
#include "common.h"
#include "mt19937_common.h"

#include <algorithm>
#include <mutex>

using namespace tf;
using namespace tf::mt;

namespace {

constexpr int RING = 1024;            // LDS words of a wave's window: 624 live + 226 new <= 850 <= RING, a power of two
constexpr int STEP = 226;             // words a step: even (a step ends on a double), at most 227 are independent
constexpr int JUMP_PARTS = 4;         // blocks that share a segment's jump, each a range of exponents
constexpr int JUMP_RANGE = (DEG + JUMP_PARTS - 1) / JUMP_PARTS;
constexpr int JUMP_LDS = JUMP_RANGE + NW - 1; // words one block's exponents reach
constexpr int JUMP_THREADS = 640;     // ten waves: one lane per word of the state
constexpr int SEG_STRIDE = JUMP_PARTS * NW; // words between two segments' states: JUMP_PARTS partial states each
constexpr uint32_t MIN_SEGMENT = 256; // words: a step of the walk crosses at most one segment start
constexpr size_t MAX_DOUBLES = (size_t)1 << 30;

__device__ __forceinline__ uint32_t ring_at(const uint32_t *ring, uint32_t k) { return ring[k & (RING - 1)]; }

// states: [G][JUMP_PARTS][624], XORed over the first nparts; out: n doubles; S: words of a segment (even); scratch:
// [G][PREFIX] or null (no jump follows); tail: null, or where the last word's successor window x[N .. N + 623] goes
// (G = 1); xor0: what the stream's very first word differs by from the window's (canonical_word0), once after a state
// is adopted.
__global__ __launch_bounds__(64) void k_mt_fill(const uint32_t *states /* tail may be it */, int nparts, double *__restrict__ out,
                                                uint32_t n_words, uint32_t S, uint32_t *__restrict__ scratch,
                                                uint32_t *tail, uint32_t xor0)
{
    __shared__ uint32_t ring[RING];
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    const uint32_t start = g * S;                       // < n_words: the host launches ceil(n_words / S) blocks
    const uint32_t len = min(S, n_words - start);       // even
    const uint32_t *st = states + (size_t)g * SEG_STRIDE;
    for (uint32_t j = lane; j < (uint32_t)NW; j += 64) {
        uint32_t v = 0;
        for (int p = 0; p < nparts; p++)
            v ^= st[p * NW + j];
        ring[j] = v;
    }
    __syncthreads();
    const uint32_t span = scratch ? max(len, (uint32_t)PREFIX) : len;
    double *o = out + start / 2;
    uint32_t *sc = scratch ? scratch + (size_t)g * PREFIX : nullptr;
    const uint32_t first = g == 0 ? xor0 : 0u;
    for (uint32_t k = 0; k < span; k += STEP) {
        uint32_t fresh[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t m = lane + 64 * q;
            if (m < (uint32_t)STEP)
                fresh[q] = next_word(ring_at(ring, k + m), ring_at(ring, k + m + 1), ring_at(ring, k + m + MW));
        }
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const uint32_t w = k + 2 * (lane + 64 * q);
            if (lane + 64 * q < (uint32_t)STEP / 2 && w < len) {
                uint32_t a = ring_at(ring, w);
                const uint32_t b = ring_at(ring, w + 1);
                if (w == 0)
                    a ^= first;
                o[w / 2] = to_double(temper(a), temper(b));
            }
        }
        if (sc) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t m = lane + 64 * q;
                if (m < (uint32_t)STEP && k + m < (uint32_t)PREFIX)
                    sc[k + m] = ring_at(ring, k + m);
            }
        }
        // the new words land on ring slots of words before k - 174: nothing this step reads
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t m = lane + 64 * q;
            if (m < (uint32_t)STEP)
                ring[(k + NW + m) & (RING - 1)] = fresh[q];
        }
        __syncthreads();
    }
    if (tail) // the ring holds x[k - 400 .. k + 623] at the loop's end, k - 226 < len <= k
        for (uint32_t j = lane; j < (uint32_t)NW; j += 64)
            tail[j] = ring_at(ring, len + j);
}

// scratch: [G][PREFIX]; rel: each set exponent minus its part's first; part_begin: [JUMP_PARTS + 1] into rel;
// states: [G][JUMP_PARTS][624], part blockIdx.x of segment blockIdx.y written.
__global__ __launch_bounds__(JUMP_THREADS) void k_mt_jump(const uint32_t *__restrict__ scratch, const uint32_t *__restrict__ rel,
                                                          const int *__restrict__ part_begin, uint32_t *__restrict__ states)
{
    __shared__ uint32_t x[JUMP_LDS];
    const uint32_t part = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const uint32_t lo = part * JUMP_RANGE;
    const uint32_t cnt = min((uint32_t)JUMP_LDS, (uint32_t)PREFIX - lo);
    const uint32_t *src = scratch + (size_t)g * PREFIX + lo;
    for (uint32_t t = tid; t < cnt; t += JUMP_THREADS)
        x[t] = src[t];
    __syncthreads();
    if (tid >= (uint32_t)NW)
        return;
    const int begin = part_begin[part], end = part_begin[part + 1];
    uint32_t acc = 0;
#pragma unroll 8
    for (int t = begin; t < end; t++)
        acc ^= x[rel[t] + tid];     // rel[t] < JUMP_RANGE and lo + rel[t] < DEG: inside the cnt staged words
    states[(size_t)g * SEG_STRIDE + part * NW + tid] = acc;
}

// state0: the window at the stream's position; states[g][0] := the window at word g * S, g < G
__global__ __launch_bounds__(64) void k_mt_walk(const uint32_t *__restrict__ state0, uint32_t *__restrict__ states, uint32_t G,
                                                uint32_t S)
{
    __shared__ uint32_t ring[RING];
    const uint32_t lane = threadIdx.x;
    for (uint32_t j = lane; j < (uint32_t)NW; j += 64)
        ring[j] = state0[j];
    __syncthreads();
    const uint32_t last = (G - 1) * S;
    for (uint32_t k = 0;; k += STEP) {
        // the ring holds x[k - 400 .. k + 623]; a segment start b with k - 226 < b <= k is met at this k alone (S >= 226)
        const uint32_t seg = k / S, b = seg * S;
        if (k - b < (uint32_t)STEP && seg < G)
            for (uint32_t j = lane; j < (uint32_t)NW; j += 64)
                states[(size_t)seg * SEG_STRIDE + j] = ring_at(ring, b + j);
        if (k >= last)
            break;
        uint32_t fresh[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t m = lane + 64 * q;
            if (m < (uint32_t)STEP)
                fresh[q] = next_word(ring_at(ring, k + m), ring_at(ring, k + m + 1), ring_at(ring, k + m + MW));
        }
        __syncthreads(); // (the window stores above read slots the new words may land on)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t m = lane + 64 * q;
            if (m < (uint32_t)STEP)
                ring[(k + NW + m) & (RING - 1)] = fresh[q];
        }
        __syncthreads();
    }
}

__global__ void k_mt_combine(const uint32_t *__restrict__ states, int nparts, uint32_t *__restrict__ out)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (uint32_t)NW)
        return;
    uint32_t v = 0;
    for (int p = 0; p < nparts; p++)
        v ^= states[p * NW + j];
    out[j] = v;
}

// phi once per process, at first use
struct CharPoly {
    int degree = 0;
    Poly phi;
    std::vector<uint32_t> terms;
};
const CharPoly &char_poly()
{
    static CharPoly cp;
    static std::once_flag once;
    std::call_once(once, [] { cp.degree = characteristic_polynomial(cp.phi, cp.terms); });
    return cp;
}

uint32_t even_up(uint64_t v) { return (uint32_t)((v + 1) & ~(uint64_t)1); }

} // namespace

struct tf_mt {
    uint32_t key[NW] = {};      // the window at the stream's position while nothing has been drawn from it
    bool on_host = true;        // key is current (else the device's states are)
    uint32_t xor0 = 0;          // key[0] ^ canonical_word0(key): the next word's correction
    bool booted = false;        // states hold the start states of the next field of `n` doubles
    size_t n = 0;
    uint32_t G = 0, S = 0;
    int nparts = 1;             // partial states per segment that the next fill XORs
    long segments_opt = 0;      // the mt_segments the plan was made under
    float bootstrap_ms = 0.f;
    DevBuf states, scratch, cur, rel, part_begin;
};

namespace {

void plan_segments(size_t n, long forced, uint32_t *G, uint32_t *S)
{
    const uint64_t N = 2 * (uint64_t)n;
    // The measured default (profiles/NOTES.md, profiles/mt_reset_bench.json): segments of about 2^15 words -- 126 at
    // 1080p, 506 at 4K; shorter ones pay more jumps than their waves save, longer ones leave one wave walking too far.
    // A field below 2^16 words is one wave's walk and never jumps.
    uint64_t want = forced > 0 ? (uint64_t)forced : std::min<uint64_t>(N >> 15, 2048);
    want = std::max<uint64_t>(1, want);
    uint32_t s = std::max(even_up((N + want - 1) / want), MIN_SEGMENT);
    *S = s;
    *G = (uint32_t)((N + s - 1) / s);
}

// the window at the stream's position into mt->cur (device)
int current_state(tf_mt *mt)
{
    if (mt->cur.bytes < NW * sizeof(uint32_t))
        TF_TRY(mt->cur.alloc(NW * sizeof(uint32_t)));
    if (mt->on_host) {
        uint32_t win[NW];
        std::copy(mt->key, mt->key + NW, win);
        win[0] = canonical_word0(mt->key);
        TF_HIP(hipMemcpyAsync(mt->cur.p, win, sizeof(win), hipMemcpyHostToDevice, stream()));
        TF_HIP(hipStreamSynchronize(stream())); // win is on this frame
        return TF_OK;
    }
    return launch("mt_combine", k_mt_combine, dim3(cdiv(NW, 256)), dim3(256), 0, mt->states.as<const uint32_t>(), mt->nparts,
                  mt->cur.as<uint32_t>());
}

int bootstrap(tf_mt *mt, size_t n)
{
    const long forced = option(OPT_MT_SEGMENTS);
    uint32_t G, S;
    plan_segments(n, forced, &G, &S);
    TF_TRY(current_state(mt)); // before the states are written again
    hipEvent_t e0 = nullptr, e1 = nullptr;
    TF_HIP(hipEventCreate(&e0));
    TF_HIP(hipEventCreate(&e1));
    int rc = TF_OK;
    do {
        if ((rc = mt->states.bytes >= (size_t)G * SEG_STRIDE * 4 ? TF_OK : mt->states.alloc((size_t)G * SEG_STRIDE * 4)) != TF_OK)
            break;
        if (G > 1) {
            if ((rc = mt->scratch.bytes >= (size_t)G * PREFIX * 4 ? TF_OK : mt->scratch.alloc((size_t)G * PREFIX * 4)) != TF_OK)
                break;
            // t^N mod phi: one polynomial per field size, the same for every segment
            const CharPoly &cp = char_poly();
            if (cp.degree != DEG) {
                rc = set_error(TF_ERR_STATE, "tf_mt: the characteristic polynomial came out with degree %d", cp.degree);
                break;
            }
            Poly p;
            std::vector<uint32_t> terms;
            jump_polynomial(2 * (uint64_t)n, cp.terms, p);
            poly_terms(p.data(), terms);
            int begin[JUMP_PARTS + 1];
            size_t t = 0;
            for (int part = 0; part < JUMP_PARTS; part++) {
                begin[part] = (int)t;
                for (; t < terms.size() && terms[t] < (uint32_t)(part + 1) * JUMP_RANGE; t++)
                    terms[t] -= (uint32_t)part * JUMP_RANGE;
            }
            begin[JUMP_PARTS] = (int)terms.size();
            if ((rc = mt->rel.upload(terms.data(), std::max<size_t>(1, terms.size()) * 4)) != TF_OK)
                break;
            if ((rc = mt->part_begin.upload(begin, sizeof(begin))) != TF_OK)
                break;
            if (hipStreamSynchronize(stream()) != hipSuccess) { // terms and begin are on this frame
                rc = set_error(TF_ERR_HIP, "tf_mt: the jump polynomial's upload failed");
                break;
            }
        }
        (void)hipEventRecord(e0, stream());
        rc = launch("mt_walk", k_mt_walk, dim3(1), dim3(64), 0, mt->cur.as<const uint32_t>(), mt->states.as<uint32_t>(), G, S);
        (void)hipEventRecord(e1, stream());
        if (rc != TF_OK)
            break;
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&mt->bootstrap_ms, e0, e1) != hipSuccess) {
            rc = set_error(TF_ERR_HIP, "tf_mt: the bootstrap failed: %s", hipGetErrorString(hipGetLastError()));
            break;
        }
    } while (0);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    TF_TRY(rc);
    mt->n = n;
    mt->G = G;
    mt->S = S;
    mt->nparts = 1;
    mt->segments_opt = forced;
    mt->booted = true;
    return TF_OK;
}

} // namespace

TF_API int tf_mt_create(tf_mt **out)
{
    TF_REQUIRE(out, "tf_mt_create: null argument");
    TF_TRY(ensure_init());
    auto h = make_handle<tf_mt>();
    TF_REQUIRE(h, "tf_mt_create: out of memory");
    seed_key(5489u, h->key);               // the generator's own default seed, until a state is set
    uint32_t win[NW];
    window_at(h->key, NW, win);
    std::copy(win, win + NW, h->key);
    h->xor0 = h->key[0] ^ canonical_word0(h->key);
    *out = h.release();
    return TF_OK;
}

TF_API void tf_mt_destroy(tf_mt *mt) { delete mt; }

TF_API int tf_mt_set_state(tf_mt *mt, const uint32_t *key, int pos)
{
    TF_REQUIRE(mt && key, "tf_mt_set_state: null argument");
    TF_REQUIRE(pos >= 0 && pos <= NW, "tf_mt_set_state: pos %d outside 0..624", pos);
    window_at(key, pos, mt->key);
    mt->xor0 = mt->key[0] ^ canonical_word0(mt->key);
    mt->on_host = true;
    mt->booted = false;
    return TF_OK;
}

TF_API int tf_mt_get_state(tf_mt *mt, uint32_t *key, int *pos)
{
    TF_REQUIRE(mt && key && pos, "tf_mt_get_state: null argument");
    if (!mt->on_host) {
        TF_TRY(current_state(mt));
        TF_HIP(hipMemcpyAsync(mt->key, mt->cur.p, sizeof(mt->key), hipMemcpyDeviceToHost, stream()));
        TF_HIP(hipStreamSynchronize(stream()));
        mt->xor0 = 0;          // a produced word: already the recurrence's own
        mt->on_host = true;    // (the device's states stay current too: booted is untouched)
    }
    std::copy(mt->key, mt->key + NW, key);
    *pos = 0;
    return TF_OK;
}

TF_API int tf_mt_random_sample_dev(tf_mt *mt, void *out_dev, size_t n)
{
    TF_REQUIRE(mt && out_dev, "tf_mt_random_sample_dev: null argument");
    TF_REQUIRE(n >= 1 && n <= MAX_DOUBLES, "tf_mt_random_sample_dev: n = %zu outside 1..2^30", n);
    TF_REQUIRE(((uintptr_t)out_dev & 7) == 0, "tf_mt_random_sample_dev: out_dev is not 8-byte aligned");
    if (!mt->booted || mt->n != n || mt->segments_opt != option(OPT_MT_SEGMENTS))
        TF_TRY(bootstrap(mt, n));
    const uint32_t N = (uint32_t)(2 * n);
    const bool jump = mt->G > 1;
    const uint32_t xor0 = mt->on_host ? mt->xor0 : 0u;
    TF_TRY(launch("mt_fill", k_mt_fill, dim3(mt->G), dim3(64), 0, mt->states.as<const uint32_t>(), mt->nparts, (double *)out_dev, N,
                  mt->S, jump ? mt->scratch.as<uint32_t>() : (uint32_t *)nullptr, jump ? (uint32_t *)nullptr : mt->states.as<uint32_t>(),
                  xor0));
    mt->on_host = false;
    mt->xor0 = 0;
    if (jump) {
        TF_TRY(launch("mt_jump", k_mt_jump, dim3(JUMP_PARTS, mt->G), dim3(JUMP_THREADS), 0, mt->scratch.as<const uint32_t>(),
                      mt->rel.as<const uint32_t>(), mt->part_begin.as<const int>(), mt->states.as<uint32_t>()));
        mt->nparts = JUMP_PARTS;
    }
    return TF_OK;
}

TF_API int tf_mt_info(tf_mt *mt, int *segments, int *segment_words, float *bootstrap_ms)
{
    TF_REQUIRE(mt, "tf_mt_info: null argument");
    if (segments)
        *segments = (int)mt->G;
    if (segment_words)
        *segment_words = (int)mt->S;
    if (bootstrap_ms)
        *bootstrap_ms = mt->bootstrap_ms;
    return TF_OK;
}

// ---- host-only entry points: no GPU call --------------------------------------------------------------------------------
TF_API int tf_mt_stage_charpoly(int *degree, uint64_t *coeff_words)
{
    TF_REQUIRE(degree && coeff_words, "tf_mt_stage_charpoly: null argument");
    const CharPoly &cp = char_poly();
    *degree = cp.degree;
    for (int w = 0; w < POLY_WORDS; w++)
        coeff_words[w] = (size_t)w < cp.phi.size() ? cp.phi[w] : 0;
    return TF_OK;
}

TF_API int tf_mt_stage_jump_poly(uint64_t J, uint64_t *out)
{
    TF_REQUIRE(out, "tf_mt_stage_jump_poly: null argument");
    const CharPoly &cp = char_poly();
    TF_REQUIRE(cp.degree == DEG, "tf_mt_stage_jump_poly: the characteristic polynomial came out with degree %d", cp.degree);
    Poly p;
    jump_polynomial(J, cp.terms, p);
    std::copy(p.begin(), p.end(), out);
    return TF_OK;
}

TF_API int tf_mt_stage_apply(const uint64_t *poly, const uint32_t *key, uint32_t *out)
{
    TF_REQUIRE(poly && key && out, "tf_mt_stage_apply: null argument");
    TF_REQUIRE((poly[POLY_WORDS - 1] >> (DEG % 64)) == 0, "tf_mt_stage_apply: the polynomial's degree is 19937 or more");
    apply_polynomial(poly, key, out);
    return TF_OK;
}

TF_API int tf_mt_stage_random_sample(const uint32_t *key, int pos, size_t n, double *out)
{
    TF_REQUIRE(key && (out || !n), "tf_mt_stage_random_sample: null argument");
    TF_REQUIRE(pos >= 0 && pos <= NW, "tf_mt_stage_random_sample: pos %d outside 0..624", pos);
    uint32_t k[NW];
    std::copy(key, key + NW, k);
    random_sample_blocks(k, &pos, n, out);
    return TF_OK;
}
