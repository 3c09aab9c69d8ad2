// trait_sums_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_traitsum.h (haplotype range masks, SNP-major words, per-SNP
// counts, bit-to-byte expansion of the genotype and heterozygote operands, the digit split and byte order of the trait operand, the
// recombination) against a plain per-individual sum, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/trait_sums_check.cpp -o trait_sums_check
// The shapes are those of tests/test_trait_sums_cpu.py: 0 to 333 individuals around the 16 of a half word, the 32 of a word and the
// 128 of a step, ranges that begin and end inside each of them and at the population's end, SNP ranges of 1 to 129 across word edges,
// 0 to 17 traits, a row stride wider than the row with garbage behind L, one-hot traits at every position of a step, quanta at the
// digit-carry edges.  Every buffer is exactly sized (rows: none behind the last individual of the range, the last row cut behind the
// last word the SNP range may read; traits: n_traits * n_ind; outputs: n_traits * n_snps and n_snps entries), so a stray access is a
// sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../geneevolve_amd/csrc/gev_traitsum.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static unsigned long long n_checked = 0, n_bad = 0;
static const int32_t edges[] = {1 << 30, -(1 << 30), 0, 1, -1, 127, -127, 128, -128, 129, -129, 32768, -32768, 32767, -32769, 8388608, -8388608, 8388607, (1 << 30) - 1, 1 - (1 << 30)};

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

// kind 0: random quanta with the edges strewn in; 1: one-hot, trait t has its one quantum at individual (first + t) of the range; 2: edge t for everybody
static void check_shape(size_t L, size_t extra, size_t s0, size_t ns, size_t i0, size_t ni, size_t nt, int kind, size_t first)
{
    const size_t stride = (L + 63) / 64 + extra;
    const std::vector<uint64_t> R = make_rows(i0 + ni, L, stride, ns ? (s0 + ns - 1) / 64 : 0);
    std::vector<int32_t> q(nt * ni);
    for (size_t t = 0; t < nt; t++)
        for (size_t i = 0; i < ni; i++) {
            const uint64_t x = rng();
            int32_t v = x % 7 == 0 ? edges[(x >> 8) % 20] : (int32_t)((int64_t)((x >> 8) % ((2ull << 30) + 1)) - (1ll << 30));
            if (kind == 1) v = i == first + t ? (int32_t)(1 + t % 120 + 256 * (3 + t % 100) - 65536 * (int32_t)(5 + t % 90) + 16777216 * (int32_t)(1 + t % 60)) * (t & 1 ? -1 : 1) : 0;
            if (kind == 2) v = edges[t % 20];
            q[t * ni + i] = v;
        }
    std::vector<int64_t> gs(nt * ns), hs(nt * ns), wg(nt * ns, 0), wh(nt * ns, 0);
    std::vector<uint32_t> het(ns), hom(ns), whet(ns, 0), whom(ns, 0);
    for (size_t i = 0; i < ni; i++)
        for (size_t j = 0; j < ns; j++) {
            const unsigned g = hap(R, stride, 2 * (i0 + i), s0 + j) + hap(R, stride, 2 * (i0 + i) + 1, s0 + j);
            whet[j] += g == 1; whom[j] += g == 2;
            for (size_t t = 0; t < nt; t++) { wg[t * ns + j] += (int64_t)g * q[t * ni + i]; wh[t * ns + j] += g == 1 ? q[t * ni + i] : 0; }
        }
    if (ni) gev_trait_sums_host(R.data(), stride, s0, ns, i0, ni, q.data(), nt, gs.data(), hs.data(), het.data(), hom.data());
    else { gs.assign(nt * ns, 0); hs.assign(nt * ns, 0); het.assign(ns, 0); hom.assign(ns, 0); }      // (the C ABI answers that one without the arithmetic)
    n_checked++;
    if (gs != wg || hs != wh || het != whet || hom != whom) {
        n_bad++;
        printf("MISMATCH: SNPs [%zu,+%zu) of %zu, individuals [%zu,+%zu), %zu traits of kind %d, stride + %zu\n", s0, ns, L, i0, ni, nt, kind, extra);
    }
    if (ni && nt) {                                                   // each output on its own
        std::vector<int64_t> only(nt * ns);
        gev_trait_sums_host(R.data(), stride, s0, ns, i0, ni, q.data(), nt, nullptr, only.data(), nullptr, nullptr);
        if (only != wh) { n_bad++; printf("MISMATCH: hetsum alone\n"); }
    }
}

int main()
{
    const size_t n_people = 340, L = 200;
    const size_t n_inds[] = {0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 333};
    const size_t snps[][2] = {{199, 1}, {56, 15}, {60, 16}, {0, 17}, {1, 63}, {64, 64}, {63, 65}, {40, 129}};
    const size_t n_traits[] = {0, 1, 3, 4, 5, 17};
    size_t k = 0;
    for (size_t ni : n_inds)
        for (size_t b : {(size_t)0, (size_t)5, (size_t)21, (size_t)70, (size_t)135, n_people}) {
            const size_t i0 = std::min(b, n_people - ni);
            for (auto& s : snps) check_shape(L, k % 2 ? 2 : 0, s[0], s[1], i0, ni, n_traits[k % 6], 0, 0), k++;
        }
    for (size_t nt : n_traits) check_shape(L, 2, 0, L, 3, 333, nt, 0, 0);
    for (size_t i0 : {(size_t)0, (size_t)3, (size_t)16, (size_t)37, (size_t)200}) {
        const size_t ni = std::min<size_t>(333, n_people - i0);
        check_shape(L, 2, 0, L, i0, ni, 128, 1, 0); check_shape(L, 0, 0, L, i0, ni, 128, 1, ni - 128);
    }
    check_shape(L, 2, 10, 70, 0, n_people, 20, 2, 0); check_shape(L, 0, 10, 70, 5, 129, 20, 2, 0);
    // the digits alone: every edge and its neighbours split and put together again
    for (int32_t e : edges)
        for (int d = -2; d <= 2; d++) {
            const int64_t v = (int64_t)e + d;
            if (v > (1 << 30) || v < -(1 << 30)) continue;
            int32_t dg[4];
            for (int j = 0; j < 4; j++) dg[j] = gev_dp_digit((int32_t)v, j);
            n_checked++;
            if (gev_dp_recombine(dg) != v || dg[0] < -128 || dg[0] > 127 || dg[1] < -128 || dg[1] > 127 || dg[2] < -128 || dg[2] > 127 || dg[3] < -65 || dg[3] > 65) { n_bad++; printf("MISMATCH: digits of %lld\n", (long long)v); }
        }
    printf("%llu shapes checked, %llu mismatches\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
