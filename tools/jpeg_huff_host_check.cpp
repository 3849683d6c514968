// The rule of the JPEG encoder's own Huffman tables (transflow_amd/csrc/jpeg_huff.h: libjpeg's jpeg_gen_optimal_table and
// jpeg_make_c_derived_tbl) run on the CPU.  Built with -fsanitize=address,undefined and run over the histograms of the
// fixtures and over hostile ones -- one symbol, none, 256 equal counts, Fibonacci counts whose code would be deeper than
// 32 bits, counts up to the selection sentinel -- it shows that no histogram makes the shared code read or write outside
// what it owns or compute anything undefined.  The work area, the counts and the results are heap allocations of exactly
// their size, so that the sanitizer sees any access beyond them.
//
//   jpeg_huff_host_check CORPUS
//
// CORPUS: one histogram per line, `name kind c0 c1 ... c255`, kind `dc` (16 entries) or `ac` (256).  Prints one line per
// histogram: `name fault bits vals entries`, fault being HuffFault's number, bits the 16 counts and vals the symbols in
// hex (`-` for none), entries the CRC-less sum of (symbol + 1) * entry over the derived table, as a check that every
// code is where jpeg_make_c_derived_tbl puts it.
#include "../transflow_amd/csrc/jpeg_huff.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

using namespace tf::jpeg;

static std::string hex(const uint8_t *p, int n)
{
    static const char digits[] = "0123456789abcdef";
    std::string out;
    for (int i = 0; i < n; i++)
        out += digits[p[i] >> 4], out += digits[p[i] & 15];
    return n ? out : "-";
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
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream fields(line);
        std::string name, kind;
        if (!(fields >> name >> kind))
            continue;
        HuffWork *w = (HuffWork *)malloc(sizeof(HuffWork));
        bool whole = true;
        for (int i = 0; i < 256; i++) {
            unsigned long v = 0;
            whole = whole && (bool)(fields >> v);
            w->freq[i] = (uint32_t)v;
        }
        if (!whole) {
            fprintf(stderr, "%s: fewer than 256 counts\n", name.c_str());
            free(w);
            return 1;
        }
        const int n_entries = kind == "dc" ? 16 : 256;
        uint8_t *bits = (uint8_t *)malloc(16), *vals = (uint8_t *)malloc(256);
        uint32_t *entries = (uint32_t *)malloc(n_entries * sizeof(uint32_t));
        int n_vals = 0;
        const int fault = gen_optimal_table(*w, bits, vals, &n_vals);
        unsigned long long sum = 0;
        if (fault == HUFF_OK) {
            huff_entries(bits, vals, entries, n_entries);
            for (int s = 0; s < n_entries; s++)
                sum += (unsigned long long)(s + 1) * entries[s];
        }
        printf("%s %d %s %s %llu\n", name.c_str(), fault, hex(bits, 16).c_str(), hex(vals, fault == HUFF_OK ? n_vals : 0).c_str(), sum);
        free(w), free(bits), free(vals), free(entries);
    }
    return 0;
}
