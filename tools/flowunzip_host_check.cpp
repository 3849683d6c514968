// The band decoder of transflow_amd/csrc/flowunzip_common.h run on the CPU: the same machine the device's lane 0 runs,
// with the wave's share of the work (window refill, match and stored copies, flushes) done by plain loops that make the
// same range checks.  Built with -fsanitize=address,undefined and run over valid and malformed bands, it shows that no
// band makes the shared code read or write outside the band's ranges.  Every buffer here is a
// heap allocation of exactly the size the decoder is entitled to, so that the sanitizer sees any access beyond it.
//
//   flowunzip_host_check CORPUS
//
// CORPUS: one case per line, `name out_bytes hex-of-the-band's-compressed-bytes` (`-` for no bytes).  Prints one line
// per case: `name verdict crc32`, the verdict being the Reject number (0: inflated whole), the CRC-32 that of the
// output (0 for a rejected band).
#include "../transflow_amd/csrc/crc32_common.h"
#include "../transflow_amd/csrc/flowunzip_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace tf::flowunzip;

// the whole band: its verdict; out: out_bytes
static uint32_t inflate_band(const uint8_t *stream, uint32_t size, uint8_t *out, uint32_t out_bytes)
{
    uint8_t *ring = (uint8_t *)malloc(RING_BYTES), *win = (uint8_t *)malloc(WINDOW_BYTES), *lengths = (uint8_t *)malloc(MAX_LENGTHS);
    Code *lit = (Code *)malloc(sizeof(Code)), *dist = (Code *)malloc(sizeof(Code));
    memset(ring, 0xA5, RING_BYTES), memset(win, 0xA5, WINDOW_BYTES), memset(lengths, 0, MAX_LENGTHS);
    memset(lit, 0, sizeof(Code)), memset(dist, 0, sizeof(Code));
    State s;
    start(s, win, size, out_bytes);
    uint32_t verdict = R_OK;
    for (;;) {
        const Action x = advance(s, *lit, *dist, lengths, ring);
        if (x.kind == A_REFILL) {
            for (uint32_t i = 0; i < x.b && i < WINDOW_BYTES; i++)
                win[i] = x.a + i < size ? stream[x.a + i] : 0;
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
                if (x.c + i < size && x.a + i < out_bytes)
                    ring[(x.a + i) & RING_MASK] = stream[x.c + i];
        } else if (x.kind == A_FLUSH || (x.kind == A_DONE && x.a == R_OK)) {
            const uint32_t upto = x.kind == A_DONE ? s.produced : s.produced & ~63u;
            if (upto > out_bytes || upto - s.flushed > RING_BYTES || s.flushed > upto) {
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

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s CORPUS\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    tf::Crc32Consts consts;
    tf::make_crc32_consts(consts);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream fields(line);
        std::string name, hex;
        unsigned long out_bytes = 0;
        if (!(fields >> name >> out_bytes >> hex))
            continue;
        if (hex == "-")
            hex.clear();
        const size_t size = hex.size() / 2;
        uint8_t *stream = (uint8_t *)malloc(size ? size : 1), *out = (uint8_t *)malloc(out_bytes ? out_bytes : 1);
        for (size_t i = 0; i < size; i++)
            stream[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        const uint32_t verdict = inflate_band(stream, (uint32_t)size, out, (uint32_t)out_bytes);
        printf("%s %u %u\n", name.c_str(), verdict, verdict == R_OK ? tf::crc32_bytes(consts, out, out_bytes) : 0u);
        free(stream), free(out);
    }
    return 0;
}
