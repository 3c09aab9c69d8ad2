// ind_scores_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_indscore.h (SNP range masks, the two planes of an individual,
// bit-to-byte expansion of the genotype and heterozygote operands, the digit split and byte order of the weight operand, the
// recombination) against a plain per-SNP loop, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/ind_scores_check.cpp -o ind_scores_check
// The shapes are those of tests/test_ind_scores_cpu.py: 150 people x 8269 SNPs; SNP ranges of 1 to 257 that begin inside a word and
// cross word, step (256 SNPs) and slice (4096 SNPs) edges, and the whole row; 1 to 150 individuals from the first, from inside the
// population and ending at the last; 0 to 17 columns; a row stride wider than the row with garbage behind L; one-hot columns at every
// byte position of a step; weights at the digit-carry edges.  Every buffer is exactly sized (rows: none behind the last individual of
// the range, the last row cut behind the last word the SNP range may read; weights: n_scores * n_snps; outputs: n_scores * n_ind), so
// a stray access is a sanitizer report.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../geneevolve_amd/csrc/gev_indscore.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static unsigned long long n_checked = 0, n_bad = 0;
static const int32_t edges[] = {0, 1, -1, 127, -127, 128, -128, 129, -129, 32768, -32768, 1 << 30, -(1 << 30)};
static const size_t n_edges = sizeof(edges) / sizeof(edges[0]);

// rows of individuals [0, i_end) over L SNPs at `stride` words, the last row cut behind word `last_word`; allele frequency by column:
// 0, 1 and in between; pad words and the bits beyond L keep their garbage
static std::vector<uint64_t> make_rows(size_t i_end, size_t L, size_t stride, size_t last_word)
{
    const size_t rows = 2 * i_end;
    std::vector<uint64_t> bits(rows ? (rows - 1) * stride + last_word + 1 : 0);
    for (size_t r = 0; r < rows; r++)
        for (size_t k = 0; k < stride && r * stride + k < bits.size(); k++) {
            uint64_t v = 0;
            for (size_t b = 0; b < 64; b++) {
                const size_t col = k * 64 + b;
                const bool one = col >= L ? rng() & 1 : col % 7 == 0 ? false : col % 7 == 1 ? true : col % 7 == 2 ? (rng() % 16 == 0) : rng() & 1;
                v |= (uint64_t)one << b;
            }
            bits[r * stride + k] = v;
        }
    return bits;
}
static unsigned hap(const std::vector<uint64_t>& bits, size_t stride, size_t h, size_t j) { return (unsigned)((bits[h * stride + j / 64] >> (j % 64)) & 1u); }

// kind 0: random weights with the edges strewn in; 1: one-hot, column t has its one weight at SNP (first + t) of the range; 2: edge t at every SNP
static void check_shape(size_t L, size_t extra, size_t s0, size_t ns, size_t i0, size_t ni, size_t nt, int kind, size_t first)
{
    const size_t stride = (L + 63) / 64 + extra;
    const std::vector<uint64_t> R = make_rows(i0 + ni, L, stride, ns ? (s0 + ns - 1) / 64 : 0);
    std::vector<int32_t> w(nt * ns);
    for (size_t t = 0; t < nt; t++)
        for (size_t j = 0; j < ns; j++) {
            const uint64_t x = rng();
            int32_t v = x % 7 == 0 ? edges[(x >> 8) % n_edges] : (int32_t)((int64_t)((x >> 8) % ((2ull << 30) + 1)) - (1ll << 30));
            if (kind == 1) v = j == first + t ? (int32_t)(1 + t % 127 + 256 * (3 + t % 100) - 65536 * (int32_t)(5 + t % 90) + 16777216 * (int32_t)(1 + t % 60)) * (t & 1 ? -1 : 1) : 0;
            if (kind == 2) v = edges[t % n_edges];
            w[t * ns + j] = v;
        }
    std::vector<int64_t> gs(nt * ni), hs(nt * ni), wg(nt * ni, 0), wh(nt * ni, 0);
    for (size_t i = 0; i < ni; i++)
        for (size_t j = 0; j < ns; j++) {
            const unsigned g = hap(R, stride, 2 * (i0 + i), s0 + j) + hap(R, stride, 2 * (i0 + i) + 1, s0 + j);
            for (size_t t = 0; t < nt; t++) { wg[t * ni + i] += (int64_t)g * w[t * ns + j]; wh[t * ni + i] += g == 1 ? w[t * ns + j] : 0; }
        }
    if (ns) gev_ind_scores_host(R.data(), stride, s0, ns, i0, ni, w.data(), nt, gs.data(), hs.data());
    else { gs.assign(nt * ni, 0); hs.assign(nt * ni, 0); }             // (the C ABI answers that one without the arithmetic)
    n_checked++;
    if (gs != wg || hs != wh) {
        n_bad++;
        printf("MISMATCH: SNPs [%zu,+%zu) of %zu, individuals [%zu,+%zu), %zu columns of kind %d, stride + %zu\n", s0, ns, L, i0, ni, nt, kind, extra);
    }
    if (ns && nt) {                                                   // each output on its own
        std::vector<int64_t> only(nt * ni);
        gev_ind_scores_host(R.data(), stride, s0, ns, i0, ni, w.data(), nt, nullptr, only.data());
        if (only != wh) { n_bad++; printf("MISMATCH: hetscore alone\n"); }
        gev_ind_scores_host(R.data(), stride, s0, ns, i0, ni, w.data(), nt, only.data(), nullptr);
        if (only != wg) { n_bad++; printf("MISMATCH: gscore alone\n"); }
    }
}

int main()
{
    const size_t n_people = 150, L = 2 * 4096 + 77;
    const size_t n_inds[] = {1, 15, 16, 17, 127, 128, 129, 150};
    const size_t snps[][2] = {{L - 1, 1}, {4095, 1}, {56, 15}, {4090, 16}, {0, 17}, {1, 63}, {64, 64}, {63, 65}, {4033, 64}, {130, 255}, {4096, 256}, {3, 256}, {250, 257}, {4000, 257}, {8100, L - 8100}, {0, 0}};
    const size_t n_scores[] = {0, 1, 3, 4, 5, 17};
    size_t k = 0;
    for (size_t ni : n_inds)
        for (size_t b : {(size_t)0, (size_t)9, n_people}) {
            const size_t i0 = std::min(b, n_people - ni);
            for (auto& s : snps) check_shape(L, k % 2 ? 2 : 0, s[0], s[1], i0, ni, n_scores[k % 6], 0, 0), k++;
        }
    for (size_t nt : n_scores) check_shape(L, 2, 0, L, 3, 40, nt, 0, 0);
    check_shape(L, 0, 0, L, 0, n_people, 5, 0, 0);
    for (size_t first : {(size_t)0, (size_t)3, (size_t)64, (size_t)100, (size_t)4096, L - 256}) {
        const size_t s0 = first >= 37 ? first - 37 : 0, ns = std::min(first + 256 + 70, L) - s0;
        check_shape(L, 2, s0, ns, 0, 40, 256, 1, first - s0); check_shape(L, 0, first, std::min(first + 256 + 70, L) - first, 5, 17, 256, 1, 0);
    }
    check_shape(L, 2, 0, 300, 10, 70, n_edges, 2, 0); check_shape(L, 0, 4000, 200, 10, 70, n_edges, 2, 0); check_shape(L, 0, 60, 5, 10, 70, n_edges, 2, 0);
    // the operand rule alone: every byte of a step names a different SNP of the step, each exactly once
    {
        std::vector<int32_t> one(256);
        for (size_t j = 0; j < 256; j++) one[j] = (int32_t)j - 128;                             // digit 0 of the weight = the SNP's index - 128
        std::vector<int> seen(256, 0);
        for (size_t q = 0; q < 4; q++)
            for (int s = 0; s < 4; s++)
                for (int j = 0; j < 4; j++) {
                    const uint32_t r = gev_is_operand_word(one.data(), 1, 0, 256, q, s, 0, 0, j);
                    for (int b = 0; b < 4; b++) seen[(int)(int8_t)(r >> (8 * b)) + 128]++;
                }
        n_checked++;
        for (size_t j = 0; j < 256; j++) if (seen[j] != 1) { n_bad++; printf("MISMATCH: SNP %zu of a step in %d bytes\n", j, seen[j]); break; }
    }
    printf("%llu shapes checked, %llu mismatches\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
