// The host side of transflow_amd/csrc/mt19937_common.h run on its own: Berlekamp-Massey over the generator's output, the
// jump polynomials, their application to a state and RandomState.random_sample in numpy's block form -- the functions
// libtfhip.so's tf_mt handle and tf_mt_stage_* call.  Built with -fsanitize=address,undefined and run on the CPU
// (tests/test_mt_ref.py).  Every buffer a case fills is a heap block of exactly its size, so that
// the sanitizer sees any access beyond it.
//
//   mt_host_check CASES
//
// CASES: one case per line.
//   charpoly            -> `charpoly DEGREE WEIGHT hex-of-the-coefficient-words`
//   jump J              -> `jump J WEIGHT hex-of-the-coefficient-words`          (t^J mod phi)
//   apply SEED POS J    -> `apply SEED POS J hex-of-624-words`   x[J .. J + 623] by the polynomial from the state described
//                          below, checked here against the stream walked word by word
//   sample SEED SKIP N  -> `sample SEED SKIP N hex-of-N-doubles` seed, SKIP 32-bit draws, then random_sample(N)
// apply's state: the seed's key with numpy's pos = POS (0..624), i.e. the window POS words into the stream whose first
// 624 words are the key; POS = 0 keeps the seed itself as word 0, the word the recurrence never produced.
#include "../transflow_amd/csrc/mt19937_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

using namespace tf::mt;

static void print_words64(const uint64_t *w, size_t n)
{
    for (size_t i = 0; i < n; i++)
        printf("%016llx", (unsigned long long)w[i]);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    Poly phi;
    std::vector<uint32_t> terms;
    const int degree = characteristic_polynomial(phi, terms);
    if (degree != DEG || terms.empty() || terms.back() != (uint32_t)DEG) {
        fprintf(stderr, "the characteristic polynomial has degree %d\n", degree);
        return 1;
    }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        std::string what;
        if (!(f >> what))
            continue;
        if (what == "charpoly") {
            uint64_t *w = (uint64_t *)calloc(POLY_WORDS, sizeof(uint64_t));
            for (int i = 0; i < POLY_WORDS; i++)
                w[i] = phi[i];
            w[POLY_WORDS - 1] &= ~((uint64_t)1 << (DEG % 64)); // the leading coefficient is implied
            printf("charpoly %d %zu ", degree, terms.size());
            print_words64(w, POLY_WORDS);
            printf("\n");
            free(w);
        } else if (what == "jump") {
            unsigned long long J;
            f >> J;
            Poly p;
            jump_polynomial(J, terms, p);
            printf("jump %llu %zu ", J, poly_weight(p));
            print_words64(p.data(), p.size());
            printf("\n");
        } else if (what == "apply") {
            unsigned seed;
            int pos;
            unsigned long long J;
            f >> seed >> pos >> J;
            uint32_t *key = (uint32_t *)malloc(NW * sizeof(uint32_t)), *win = (uint32_t *)malloc(NW * sizeof(uint32_t)),
                     *out = (uint32_t *)malloc(NW * sizeof(uint32_t));
            seed_key(seed, key);
            window_at(key, pos, win);
            Poly p;
            jump_polynomial(J, terms, p);
            apply_polynomial(p.data(), win, out);
            std::vector<uint32_t> x((size_t)J + NW);
            raw_stream(win, x.size(), x.data());
            if (J >= 1 && memcmp(out, x.data() + J, NW * sizeof(uint32_t)) != 0) {
                fprintf(stderr, "apply %u %d %llu: the polynomial and the walked stream differ\n", seed, pos, J);
                return 1;
            }
            printf("apply %u %d %llu ", seed, pos, J);
            for (int j = 0; j < NW; j++)
                printf("%08x", out[j]);
            printf("\n");
            free(key);
            free(win);
            free(out);
        } else if (what == "sample") {
            unsigned seed;
            size_t skip, n;
            f >> seed >> skip >> n;
            uint32_t *key = (uint32_t *)malloc(NW * sizeof(uint32_t));
            seed_key(seed, key);
            int pos = NW;
            // SKIP 32-bit draws: through the position form, so that the block form below starts inside a block
            uint32_t *win = (uint32_t *)malloc(NW * sizeof(uint32_t));
            std::vector<uint32_t> x(skip + 2 * (size_t)NW);
            raw_stream(key, x.size(), x.data());
            const size_t at = (size_t)NW + skip;            // the stream word the first double starts at
            const size_t block = at / NW * NW;              // the numpy block it lies in
            memcpy(key, x.data() + (at % NW == 0 ? block - NW : block), NW * sizeof(uint32_t));
            pos = at % NW == 0 ? NW : (int)(at % NW);
            double *out = (double *)malloc((n ? n : 1) * sizeof(double));
            random_sample_blocks(key, &pos, n, out);
            // the same doubles from the window at that word, by position
            window_at(x.data() + (at % NW == 0 ? block - NW : block), at % NW == 0 ? NW : (int)(at % NW), win);
            std::vector<uint32_t> y(2 * n + NW);
            raw_stream(win, y.size(), y.data());
            for (size_t i = 0; i < n; i++)
                if (to_double(temper(y[2 * i]), temper(y[2 * i + 1])) != out[i]) {
                    fprintf(stderr, "sample %u %zu %zu: block form and position form differ at %zu\n", seed, skip, n, i);
                    return 1;
                }
            printf("sample %u %zu %zu ", seed, skip, n);
            for (size_t i = 0; i < n; i++) {
                uint64_t bits;
                memcpy(&bits, &out[i], 8);
                printf("%016llx", (unsigned long long)bits);
            }
            printf("\n");
            free(key);
            free(win);
            free(out);
        } else {
            fprintf(stderr, "unknown case %s\n", what.c_str());
            return 1;
        }
    }
    return 0;
}
