// The CRC-32 of transflow_amd/csrc/crc32_common.h run on the CPU: the same functions the device codecs call, with a
// wave's 64 lanes done by a plain loop.  Built with -fsanitize=address,undefined and run over messages of the lengths
// where the slices change shape, it holds the shared arithmetic to zlib (tests/test_flowunzip_ref.py; DESIGN.md section
// 16).  A message is a heap allocation of exactly its size, so that the sanitizer sees any access beyond it.
//
//   crc32_host_check CORPUS
//
// CORPUS: one case per line, `name hex-of-the-message` (`-` for no bytes).  Prints one line per case, `name` and the
// message's CRC-32 computed four ways: the table over all bytes (crc32_bytes); 64 plain slices, each moved in front of
// the bytes behind it and XORed (k_fz_count's); 64 slices of whole dwords, likewise (k_png_pack's, k_fu_crc's); two
// bands split at n / 2, each from 64 slices, the first moved in front of the second (k_fz_scan's, k_fu_finish's).
#include "../transflow_amd/csrc/crc32_common.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

using namespace tf;

constexpr uint32_t LANES = 64;

// bytes [0, n) in LANES slices of `slice` bytes, as a wave does them
static uint32_t by_slices(const Crc32Consts &c, const uint8_t *p, uint32_t n, uint32_t slice)
{
    uint32_t all = 0;
    for (uint32_t lane = 0; lane < LANES; lane++) {
        const uint32_t begin = lane * slice < n ? lane * slice : n, end = begin + slice < n ? begin + slice : n;
        uint32_t reg = 0xFFFFFFFFu;
        for (uint32_t j = begin; j < end; j++)
            reg = crc32_update(reg, p[j], c.crc);
        all ^= crc32_shift(~reg, n - end, c.x2n);
    }
    return all;
}

static uint32_t plain_slice(uint32_t n) { return (n + LANES - 1) / LANES; }
static uint32_t dword_slice(uint32_t n) { return (plain_slice(n) + 3) & ~3u; }

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
    Crc32Consts *c = (Crc32Consts *)malloc(sizeof(Crc32Consts));
    make_crc32_consts(*c);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream fields(line);
        std::string name, hex;
        if (!(fields >> name >> hex))
            continue;
        if (hex == "-")
            hex.clear();
        const uint32_t n = (uint32_t)(hex.size() / 2), half = n / 2;
        uint8_t *p = (uint8_t *)malloc(n ? n : 1);
        for (uint32_t i = 0; i < n; i++)
            p[i] = (uint8_t)strtoul(hex.substr(2 * (size_t)i, 2).c_str(), nullptr, 16);
        const uint32_t front = by_slices(*c, p, half, plain_slice(half)), back = by_slices(*c, p + half, n - half, plain_slice(n - half));
        printf("%s %u %u %u %u\n", name.c_str(), crc32_bytes(*c, p, n), by_slices(*c, p, n, plain_slice(n)),
               by_slices(*c, p, n, dword_slice(n)), crc32_shift(front, n - half, c->x2n) ^ back);
        free(p);
    }
    free(c);
    return 0;
}
