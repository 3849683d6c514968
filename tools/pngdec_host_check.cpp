// The banded-PNG decoder of transflow_amd/csrc/pngdec_common.h and flowunzip_common.h run on the CPU: the walk the host
// runs, the machine the device's lane 0 runs, and the waves' share of the work (the chunk CRCs by 64 slices, window
// refill, match and stored copies, flushes, the rows' sums, the unfilter) done by plain loops that make the same range
// checks.  Built with -fsanitize=address,undefined and run over valid, malformed and hostile files, it shows that no file
// makes the shared code read or write outside what the decoder is entitled to.  Every buffer
// here -- the file, the band table, each band's slot, the pixels -- is a heap allocation of exactly that size, so that
// the sanitizer sees any access beyond it.
//
//   pngdec_host_check LIST
//
// LIST: one case per line, `name path`.  Prints one line per case:
// `name reject indexed why_not width height band_rows n_bands crc32`, `reject` the reject word (0: none), the CRC-32 that
// of the RGB pixels (0 unless the file is indexed and accepted).
#include "../transflow_amd/csrc/crc32_common.h"
#include "../transflow_amd/csrc/flowunzip_common.h"
#include "../transflow_amd/csrc/pngdec_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace tf;
using namespace tf::pngdec;
namespace fu = tf::flowunzip;

// one band: its verdict (a flowunzip Reject); out: out_bytes
static uint32_t inflate_band(const uint8_t *stream, uint32_t size, uint8_t *out, uint32_t out_bytes)
{
    using namespace fu;
    uint8_t *ring = (uint8_t *)malloc(RING_BYTES), *win = (uint8_t *)malloc(WINDOW_BYTES), *lengths = (uint8_t *)malloc(MAX_LENGTHS);
    Code *lit = (Code *)malloc(sizeof(Code)), *dist = (Code *)malloc(sizeof(Code));
    memset(ring, 0xA5, RING_BYTES), memset(win, 0xA5, WINDOW_BYTES), memset(lengths, 0, MAX_LENGTHS);
    memset(lit, 0, sizeof(Code)), memset(dist, 0, sizeof(Code));
    State s;
    start(s, win, size, out_bytes);
    uint32_t verdict = fu::R_OK;
    for (;;) {
        const Action x = advance(s, *lit, *dist, lengths, ring);
        if (x.kind == A_REFILL) {
            for (uint32_t i = 0; i < x.b && i < WINDOW_BYTES; i++)
                win[i] = (x.a <= size && i < size - x.a) ? stream[x.a + i] : 0;
        } else if (x.kind == A_MATCH) {
            const uint32_t at = x.a, len = x.b, d = x.c;
            if (d == 0 || d > at || d > RING_BYTES || len > 258 || len > out_bytes - (at < out_bytes ? at : out_bytes)) {
                verdict = R_DISTANCE;
                break;
            }
            uint8_t v[258];
            for (uint32_t j = 0; j < len; j++)
                v[j] = ring[(at - d + (j < d ? j : j % d)) & RING_MASK];
            for (uint32_t j = 0; j < len; j++)
                ring[(at + j) & RING_MASK] = v[j];
        } else if (x.kind == A_STORED) {
            for (uint32_t i = 0; i < x.b && i < STORED_CHUNK; i++)
                if (x.c <= size && i < size - x.c && x.a <= out_bytes && i < out_bytes - x.a)
                    ring[(x.a + i) & RING_MASK] = stream[x.c + i];
        } else if (x.kind == A_FLUSH || (x.kind == A_DONE && x.a == fu::R_OK)) {
            const uint32_t upto = x.kind == A_DONE ? s.produced : s.produced & ~63u;
            if (upto > out_bytes || s.flushed > upto || upto - s.flushed > RING_BYTES) {
                verdict = R_OVERRUN;
                break;
            }
            for (uint32_t i = s.flushed; i < upto; i++)
                out[i] = ring[i & RING_MASK];
            s.flushed = upto;
        }
        if (x.kind == A_DONE) {
            verdict = x.a;
            break;
        }
    }
    free(ring), free(win), free(lengths), free(lit), free(dist);
    return verdict;
}

// a band chunk's CRC-32 (type and data) as a wave computes it: 64 slices, each moved in front of the bytes behind it
static uint32_t crc_by_slices(const Crc32Consts &c, const uint8_t *p, uint32_t n)
{
    const uint32_t slice = (n + 63) / 64;
    uint32_t all = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t begin = lane * slice < n ? lane * slice : n, end = begin + slice < n ? begin + slice : n;
        uint32_t reg = 0xFFFFFFFFu;
        for (uint32_t j = begin; j < end; j++)
            reg = crc32_update(reg, p[j], c.crc);
        all ^= crc32_shift(~reg, n - end, c.x2n);
    }
    return all;
}

struct Result {
    uint32_t reject = 0, crc = 0;
    Layout l;
};

static Result decode(const Crc32Consts &consts, const uint8_t *file, size_t n)
{
    Result r;
    fu::Code *lit = (fu::Code *)malloc(sizeof(fu::Code)), *dist = (fu::Code *)malloc(sizeof(fu::Code));
    uint8_t *lengths = (uint8_t *)malloc(fu::MAX_LENGTHS);
    memset(lit, 0, sizeof(fu::Code)), memset(dist, 0, sizeof(fu::Code)), memset(lengths, 0, fu::MAX_LENGTHS);
    r.reject = walk(file, n, MAX_DIM, MAX_DIM, r.l, nullptr, nullptr, 0, *lit, *dist, lengths);
    uint32_t *off = nullptr, *size = nullptr;
    uint8_t *pix = nullptr;
    std::vector<uint8_t *> slots;
    const Layout &l = r.l;
    if (r.reject == R_OK && l.indexed) {
        off = (uint32_t *)malloc(l.n_bands * sizeof(uint32_t)), size = (uint32_t *)malloc(l.n_bands * sizeof(uint32_t));
        Layout again;
        r.reject = walk(file, n, MAX_DIM, MAX_DIM, again, off, size, l.n_bands, *lit, *dist, lengths);
    }
    if (r.reject == R_OK && l.indexed)
        r.reject = check_small_crcs(file, n, l, consts);
    if (r.reject == R_OK && l.indexed) {
        for (uint32_t b = 0; b < l.n_bands && r.reject == R_OK; b++) {
            if (off[b] < 4 || off[b] > n || size[b] > n - off[b] || n - off[b] - size[b] < 4 ||
                crc_by_slices(consts, file + off[b] - 4, size[b] + 4) != be32(file + off[b] + size[b]))
                r.reject = make_reject(R_CHUNK_CRC, l.first_band_chunk + b);
        }
    }
    const uint64_t L = row_bytes(l.width);
    if (r.reject == R_OK && l.indexed) {
        for (uint32_t b = 0; b < l.n_bands; b++) {
            const uint32_t out_bytes = (uint32_t)(band_row_count(l, b) * L);
            slots.push_back((uint8_t *)malloc(out_bytes));
            memset(slots.back(), 0xA5, out_bytes);
            const uint32_t verdict = inflate_band(file + off[b], size[b], slots.back(), out_bytes);
            if (verdict != fu::R_OK && r.reject == R_OK)
                r.reject = make_reject(R_BAND + verdict, b);
        }
    }
    if (r.reject == R_OK && l.indexed) {
        uint32_t *rowsums = (uint32_t *)malloc(2 * (size_t)l.height * sizeof(uint32_t));
        for (uint32_t y = 0; y < l.height; y++) {
            const uint8_t *row = slots[y / l.band_rows] + (size_t)(y % l.band_rows) * L;
            if (row[0] > 4 && r.reject == R_OK)
                r.reject = make_reject(R_FILTER_TYPE, y);
            uint64_t s1 = 0, s2 = 0;
            for (uint64_t j = 0; j < L; j++)
                s1 += row[j], s2 += row[j] * (L - j);
            rowsums[2 * (size_t)y] = (uint32_t)(s1 % 65521), rowsums[2 * (size_t)y + 1] = (uint32_t)(s2 % 65521);
        }
        if (r.reject == R_OK && adler_of_rows(rowsums, l.height, L) != l.adler)
            r.reject = R_ADLER;
        free(rowsums);
    }
    if (r.reject == R_OK && l.indexed) {
        const size_t n_row = 3 * (size_t)l.width;
        pix = (uint8_t *)malloc(n_row * l.height);
        for (uint32_t y = 0; y < l.height; y++) {
            const uint8_t *row = slots[y / l.band_rows] + (size_t)(y % l.band_rows) * L;
            uint8_t *cur = pix + y * n_row;
            const uint8_t *above = y ? cur - n_row : nullptr;
            for (size_t i = 0; i < n_row; i++) {
                const uint32_t a = i >= 3 ? cur[i - 3] : 0, b = above ? above[i] : 0, c = (above && i >= 3) ? above[i - 3] : 0;
                cur[i] = (uint8_t)unfilter_byte(row[0], row[1 + i], a, b, c);
            }
        }
        r.crc = crc32_bytes(consts, pix, n_row * l.height);
    }
    for (uint8_t *s : slots)
        free(s);
    free(pix), free(off), free(size), free(lit), free(dist), free(lengths);
    return r;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s LIST\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    Crc32Consts consts;
    make_crc32_consts(consts);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream fields(line);
        std::string name, path;
        if (!(fields >> name >> path))
            continue;
        std::ifstream f(path, std::ios::binary);
        if (!f) {
            fprintf(stderr, "cannot read %s\n", path.c_str());
            return 2;
        }
        const std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        uint8_t *file = (uint8_t *)malloc(bytes.size() ? bytes.size() : 1);
        memcpy(file, bytes.data(), bytes.size());
        const Result r = decode(consts, file, bytes.size());
        printf("%s %u %u %u %u %u %u %u %u\n", name.c_str(), r.reject, r.l.indexed, r.l.why_not, r.l.width, r.l.height, r.l.band_rows, r.l.n_bands,
               r.crc);
        free(file);
    }
    return 0;
}
