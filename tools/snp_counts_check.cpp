// snp_counts_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_snpcount.h (the vertical genotype counter) against a plain
// per-bit count, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/snp_counts_check.cpp -o snp_counts_check
// The shapes are those of tests/test_snp_counts_cpu.py: individuals around the counter's period F, loci around word and chunk edges,
// a row stride wider than the row with garbage behind it, SNP ranges that begin and end inside a word.  Every buffer is exactly
// sized (rows: only the words the range may read are allocated past the last row's range), so a stray access is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../geneevolve_amd/csrc/gev_snpcount.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static unsigned long long n_checked = 0, n_bad = 0;

static void check(size_t n_ind, size_t L, size_t extra_words, size_t s0, size_t ns)
{
    const size_t w = (L + 63) / 64, stride = w + extra_words, rows = 2 * n_ind;
    // the last row is cut behind the last word of the SNP range: nothing beyond may be read
    const size_t last_word = ns ? (s0 + ns - 1) / 64 : 0;
    std::vector<uint64_t> bits(rows ? (rows - 1) * stride + last_word + 1 : 0);
    for (size_t r = 0; r < rows; r++)
        for (size_t k = 0; k < stride && r * stride + k < bits.size(); k++) {
            uint64_t v = rng();
            const size_t col = (k * 64) % (L ? L : 1);                 // allele frequency by column: 0, 1 and in between
            if (col % 7 == 0) v = 0; else if (col % 7 == 1) v = ~0ull; else if (col % 7 == 2) v &= rng() & rng();
            bits[r * stride + k] = v;                                  // pad words and the bits beyond L keep their garbage
        }
    std::vector<uint32_t> het(ns), hom(ns), want_het(ns, 0), want_hom(ns, 0);
    for (size_t i = 0; i < n_ind; i++)
        for (size_t j = 0; j < ns; j++) {
            const size_t g = s0 + j;
            const unsigned a = (unsigned)(bits[2 * i * stride + g / 64] >> (g % 64)) & 1u, b = (unsigned)(bits[(2 * i + 1) * stride + g / 64] >> (g % 64)) & 1u;
            want_het[j] += a ^ b; want_hom[j] += a & b;
        }
    gev_snpc_count_rows_host(bits.data(), stride, n_ind, s0, ns, het.data(), hom.data());
    n_checked++;
    if (het != want_het || hom != want_hom) { n_bad++; printf("MISMATCH: %zu individuals x %zu loci, stride + %zu, SNPs [%zu,%zu)\n", n_ind, L, extra_words, s0, s0 + ns); }
}

int main()
{
    const size_t F = GEV_SNPC_F;
    const size_t n_inds[] = {0, 1, 2, F - 1, F, F + 1, 3 * F + 5};
    const size_t loci[] = {1, 31, 32, 33, 127, 128, 129, 5000};
    const size_t ranges[][2] = {{5, 17}, {31, 33}, {63, 65}, {70, 120}, {100, 140}, {127, 129}, {64, 128}, {130, 4097}, {4999, 5000}};
    for (size_t n : n_inds)
        for (size_t L : loci)
            for (size_t extra = 0; extra <= 3; extra += 3) {
                check(n, L, extra, 0, L); check(n, L, extra, 0, 1); check(n, L, extra, L - 1, 1); check(n, L, extra, L, 0); check(n, L, extra, L / 2, L - L / 2);
                for (auto& r : ranges) if (r[1] <= L) check(n, L, extra, r[0], r[1] - r[0]);
            }
    printf("%llu shapes checked, %llu mismatches (K = %d, F = %u)\n", n_checked, n_bad, GEV_SNPC_K, GEV_SNPC_F);
    return n_bad ? 1 : 0;
}
