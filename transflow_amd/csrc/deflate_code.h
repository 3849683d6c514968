// What the two deflate coders (flowzip.hip, png.hip) share beyond RFC 1951's alphabets: the size of a band's stored form,
// and a literal/length code built from a histogram by one work-group (k_fz_table, k_png_table).  tests/flowzip_ref.py's
// stored_bytes, build_lengths and canonical_codes are the numpy statement of the same rules.
#pragma once
#include "common.h"
#include "deflate_tables.h"

namespace tf {
namespace deflate {

// a stored band: blocks of at most 65535 bytes, each behind 00, its length and the length's complement
constexpr uint32_t STORED_MAX = 65535;
__host__ __device__ inline uint64_t stored_bytes(uint64_t n) { return n + 5 * ((n + STORED_MAX - 1) / STORED_MAX); }

constexpr int MAX_CODE_BITS = 15;
constexpr int HUFFMAN_BLOCK = 512; // the threads of a work-group that calls huffman_build: one per symbol at the least

// n of 3 .. 258 -> k of its length symbol 257 + k
__host__ __device__ __forceinline__ int length_symbol(int n)
{
    int k = N_LENGTH_SYMBOLS - 1;
    if (n < MAX_MATCH) {
        k = 0;
        while (k + 1 < N_LENGTH_SYMBOLS - 1 && LENGTH_BASE[k + 1] <= n)
            k++;
    }
    return k;
}

// a Huffman code goes into the stream from its most significant bit
__device__ __forceinline__ uint32_t reverse_bits(uint32_t code, int n)
{
    return n ? __brev(code) >> (32 - n) : 0;
}

// The LDS the build works over; the caller owns it, fills `w` with the symbols' weights (0: unused) before the call and
// reads `len` and `code` after it.
struct HuffmanLds {
    uint32_t w[N_SYMBOLS];
    int leaf[N_SYMBOLS];              // the used symbols by (weight, symbol)
    int rank[N_SYMBOLS];              // a used symbol's place in leaf
    uint32_t node_w[2 * N_SYMBOLS];   // leaves in sorted order, then the internal nodes in the order made
    int parent[2 * N_SYMBOLS];
    int len[N_SYMBOLS];               // out: the code lengths, 0 for an unused symbol
    uint32_t code[N_SYMBOLS];         // out: the canonical codes
    uint32_t next[MAX_CODE_BITS + 2];
    int used, longest;
};

// Every thread of the work-group calls it (blockDim.x >= N_SYMBOLS); returns how often the weights were halved to
// bring the code within MAX_CODE_BITS.  The used symbols are ranked by (weight, symbol); one thread merges the two
// smallest from the two queues -- sorted leaves, internal nodes in the order they were made, which is the order of the
// key (weight, 1000 + k) -- and the symbols walk to the root for their depths; then the canonical codes.
__device__ __forceinline__ uint32_t huffman_build(HuffmanLds &s, int tid)
{
    uint32_t repairs = 0;
    for (;;) {
        if (tid == 0)
            s.used = 0, s.longest = 0;
        __syncthreads();
        // ---- rank the used symbols by (weight, symbol)
        if (tid < N_SYMBOLS && s.w[tid]) {
            const uint32_t w = s.w[tid];
            int rank = 0;
            for (int o = 0; o < N_SYMBOLS; o++) {
                const uint32_t v = s.w[o];
                rank += (v && (v < w || (v == w && o < tid))) ? 1 : 0;
            }
            s.rank[tid] = rank, s.leaf[rank] = tid, s.node_w[rank] = w;
            atomicAdd(&s.used, 1);
        }
        __syncthreads();
        const int used = s.used;
        // ---- merge the two smallest on (weight, order): a leaf's order is its symbol, the k-th internal node's 1000 + k,
        // so of equal weights the leaf goes first and of two internal nodes the older
        // (the heads of the two queues are kept in registers, the leaves' one load ahead: the loop is a chain of LDS
        // round trips otherwise, and a frame whose counts span six decades goes through it ten times)
        if (tid == 0) {
            int leaf = 0, inner = used, made = used; // the next of either queue, the next node to make
            uint32_t leaf_w = s.node_w[0], leaf_next = s.node_w[1], inner_w = 0; // (read only while leaf < used, inner < made)
            for (int k = 0; k + 1 < used; k++) {
                int pick[2];
                uint32_t sum = 0;
                for (int p = 0; p < 2; p++) {
                    const bool take_leaf = leaf < used && (inner >= made || leaf_w <= inner_w);
                    if (take_leaf) {
                        sum += leaf_w, pick[p] = leaf++;
                        leaf_w = leaf_next, leaf_next = s.node_w[leaf + 1]; // (inside the array: leaf + 1 <= used < 2 N)
                    } else {
                        sum += inner_w, pick[p] = inner++;
                        if (inner < made)
                            inner_w = s.node_w[inner];
                    }
                }
                s.node_w[made] = sum;
                s.parent[pick[0]] = s.parent[pick[1]] = made;
                if (inner == made) // the node just made is the head of its queue
                    inner_w = sum;
                made++;
            }
        }
        __syncthreads();
        if (tid < N_SYMBOLS) {
            int depth = 0;
            if (s.w[tid]) {
                const int root = 2 * used - 2;
                for (int i = s.rank[tid]; i < root && depth < 2 * N_SYMBOLS; i = s.parent[i])
                    depth++;
                if (used == 1)
                    depth = 1; // (never: the first byte and end-of-block are always there)
                atomicMax(&s.longest, depth);
            }
            s.len[tid] = depth;
        }
        __syncthreads();
        if (s.longest <= MAX_CODE_BITS)
            break;
        if (tid < N_SYMBOLS && s.w[tid])
            s.w[tid] = max(1u, s.w[tid] >> 1);
        repairs++;
        __syncthreads();
    }
    // ---- canonical codes, RFC 1951 3.2.2
    if (tid == 0) {
        uint32_t count[MAX_CODE_BITS + 2] = {};
        for (int sym = 0; sym < N_SYMBOLS; sym++)
            count[s.len[sym]]++;
        count[0] = 0;
        uint32_t code = 0;
        s.next[0] = 0;
        for (int bits = 1; bits <= MAX_CODE_BITS; bits++) {
            code = (code + count[bits - 1]) << 1;
            s.next[bits] = code;
        }
    }
    __syncthreads();
    if (tid < N_SYMBOLS) {
        const int len = s.len[tid];
        uint32_t before = 0;
        for (int o = 0; o < tid; o++)
            before += s.len[o] == len ? 1 : 0;
        s.code[tid] = len ? s.next[len] + before : 0;
    }
    __syncthreads();
    return repairs;
}

} // namespace deflate
} // namespace tf
