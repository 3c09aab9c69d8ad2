// pair_counts_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_paircount.h (range masks, bit planes, bit-to-byte expansion,
// finishing formulas, weighted sums) against a plain per-locus count, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/pair_counts_check.cpp -o pair_counts_check
// The shapes are those of tests/test_pair_counts_cpu.py: individuals around the 16-row fragment, loci around word edges, a row stride
// wider than the row with garbage behind it, SNP ranges that begin and end inside a word, ranges of individuals that are equal,
// disjoint, overlapping and of different lengths.  Every buffer is exactly sized (rows: the last row is cut behind the last word the
// range may read; outputs: n_ind, n_a * n_b and n_snps entries), so a stray access is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../geneevolve_amd/csrc/gev_paircount.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static unsigned long long n_checked = 0, n_bad = 0;

static void check(size_t n_ind, size_t L, size_t extra_words, size_t s0, size_t ns, size_t a0, size_t na, size_t b0, size_t nb)
{
    const size_t w = (L + 63) / 64, stride = w + extra_words, rows = 2 * n_ind;
    const size_t last_word = ns ? (s0 + ns - 1) / 64 : 0;
    std::vector<uint64_t> bits(rows ? (rows - 1) * stride + last_word + 1 : 0);
    for (size_t r = 0; r < rows; r++)
        for (size_t k = 0; k < stride && r * stride + k < bits.size(); k++) {
            uint64_t v = rng();
            const size_t col = (k * 64) % (L ? L : 1);                 // allele frequency by column: 0, 1 and in between
            if (col % 7 == 0) v = 0; else if (col % 7 == 1) v = ~0ull; else if (col % 7 == 2) v &= rng() & rng();
            bits[r * stride + k] = v;                                  // pad words and the bits beyond L keep their garbage
        }
    auto g = [&](size_t i, size_t j) { return (unsigned)((bits[2 * i * stride + j / 64] >> (j % 64)) & 1u) + (unsigned)((bits[(2 * i + 1) * stride + j / 64] >> (j % 64)) & 1u); };
    std::vector<uint32_t> het(n_ind), hom(n_ind), want_het(n_ind, 0), want_hom(n_ind, 0);
    std::vector<uint32_t> hh(na * nb), oh(na * nb), dot(na * nb), want_hh(na * nb, 0), want_oh(na * nb, 0), want_dot(na * nb, 0);
    std::vector<uint32_t> weight(ns);
    for (size_t j = 0; j < ns; j++) weight[j] = j % 3 ? (uint32_t)rng() : 0xFFFFFFFFu;
    std::vector<uint64_t> want_ws(n_ind, 0), ws(n_ind, 0);
    for (size_t i = 0; i < n_ind; i++)
        for (size_t j = s0; j < s0 + ns; j++) { want_het[i] += g(i, j) == 1; want_hom[i] += g(i, j) == 2; want_ws[i] += (uint64_t)weight[j - s0] * g(i, j); }
    for (size_t i = 0; i < na; i++)
        for (size_t k = 0; k < nb; k++)
            for (size_t j = s0; j < s0 + ns; j++) {
                const unsigned gi = g(a0 + i, j), gk = g(b0 + k, j);
                want_hh[i * nb + k] += gi == 1 && gk == 1; want_oh[i * nb + k] += gi + gk == 2 && gi != 1; want_dot[i * nb + k] += gi * gk;
            }
    gev_pc_counts_host(bits.data(), stride, n_ind, s0, ns, a0, na, b0, nb, het.data(), hom.data(), hh.data(), oh.data(), dot.data());
    // the weighted sum as the device's preparation pass takes it: word by word of the range
    for (size_t i = 0; i < n_ind && ns; i++)
        for (size_t wd = s0 / 64; wd <= (s0 + ns - 1) / 64; wd++) {
            uint64_t x, y;
            gev_pc_planes(bits[2 * i * stride + wd], bits[(2 * i + 1) * stride + wd], gev_pc_range_mask(wd, s0, s0 + ns), x, y);
            ws[i] += gev_pc_weighted(x, y, weight.data(), (ptrdiff_t)(64 * wd) - (ptrdiff_t)s0);
        }
    n_checked++;
    if (het != want_het || hom != want_hom || hh != want_hh || oh != want_oh || dot != want_dot || ws != want_ws) {
        n_bad++;
        printf("MISMATCH: %zu individuals x %zu loci, stride + %zu, SNPs [%zu,%zu), a [%zu,+%zu) b [%zu,+%zu)\n", n_ind, L, extra_words, s0, s0 + ns, a0, na, b0, nb);
    }
}

int main()
{
    const size_t n_inds[] = {1, 2, 15, 16, 17, 33, 70};
    const size_t loci[] = {1, 31, 64, 65, 127, 129, 5000};
    const size_t ranges[][2] = {{5, 17}, {31, 33}, {63, 65}, {70, 120}, {100, 140}, {127, 129}, {64, 128}, {130, 4097}, {4999, 5000}};
    for (size_t n : n_inds)
        for (size_t L : loci)
            for (size_t extra = 0; extra <= 3; extra += 3) {
                const size_t h = n / 2;
                check(n, L, extra, 0, L, 0, n, 0, n); check(n, L, extra, 0, 1, 0, n, 0, n); check(n, L, extra, L - 1, 1, 0, 1, n - 1, 1);
                check(n, L, extra, L, 0, 0, n, 0, n); check(n, L, extra, L / 2, L - L / 2, 0, h, h, n - h); check(n, L, extra, 0, L, h, n - h, 0, h + 1);
                check(n, L, extra, 0, L, 0, 0, 0, n);
                for (auto& r : ranges) if (r[1] <= L) check(n, L, extra, r[0], r[1] - r[0], n / 3, n - n / 3, 0, n - n / 4);
            }
    // the extremes: everybody 1/1 over 2^16 + 3 loci (dot = 4 n_snps), weights of 2^32 - 1 (a sum that needs 64 bits)
    {
        const size_t L = 65539, w = (L + 63) / 64;
        std::vector<uint64_t> bits(4 * w, ~0ull);
        uint32_t het[2], hom[2], hh[4], oh[4], dot[4];
        gev_pc_counts_host(bits.data(), w, 2, 0, L, 0, 2, 0, 2, het, hom, hh, oh, dot);
        std::vector<uint32_t> weight(L, 0xFFFFFFFFu);
        uint64_t ws = 0;
        for (size_t wd = 0; wd < w; wd++) { uint64_t x, y; gev_pc_planes(bits[wd], bits[w + wd], gev_pc_range_mask(wd, 0, L), x, y); ws += gev_pc_weighted(x, y, weight.data(), (ptrdiff_t)(64 * wd)); }
        n_checked++;
        if (het[0] || hom[1] != L || hh[1] || oh[2] || dot[3] != 4 * L || ws != 2ull * L * 0xFFFFFFFFull) { n_bad++; printf("MISMATCH: the extremes\n"); }
    }
    printf("%llu shapes checked, %llu mismatches\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
