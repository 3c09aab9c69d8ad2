// ld_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_ldcount.h (haplotype range masks, SNP-major words, per-SNP counts,
// bit-to-byte expansion of both operands, the r^2 quantum, windows) against a plain per-haplotype count, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/ld_check.cpp -o ld_check
// The shapes are those of tests/test_ld_cpu.py: individuals around the 16-row fragment and the 32 individuals of a word, ranges of
// individuals that begin and end inside a word and at the population's end, SNP blocks around the fragment and the tile that are
// equal, disjoint, overlapping and rectangular, two chromosomes, a row stride wider than the row with garbage behind L, windows of
// 0, 1, 50 SNPs and the whole chromosome.  Every buffer is exactly sized (rows: none behind the last individual of the range, the last
// row cut behind the last word a side or window may read; outputs: n_a * n_b, n_a and n_b entries), so a stray access is a sanitizer
// report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../geneevolve_amd/csrc/gev_ldcount.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static unsigned long long n_checked = 0, n_bad = 0, n_mono = 0, n_poly = 0, n_between = 0;

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

static void check_block(size_t La, size_t Lb, size_t extra, size_t a0, size_t na, size_t b0, size_t nb, size_t i0, size_t ni, bool two_chromosomes)
{
    const size_t sa = (La + 63) / 64 + extra, sb = (Lb + 63) / 64 + extra;
    const size_t last_a = two_chromosomes ? (na ? (a0 + na - 1) / 64 : 0) : std::max(na ? (a0 + na - 1) / 64 : 0, nb ? (b0 + nb - 1) / 64 : 0);
    const std::vector<uint64_t> A = make_rows(i0 + ni, La, sa, last_a);
    const std::vector<uint64_t> B2 = two_chromosomes ? make_rows(i0 + ni, Lb, sb, nb ? (b0 + nb - 1) / 64 : 0) : std::vector<uint64_t>();
    const std::vector<uint64_t>& B = two_chromosomes ? B2 : A;
    const size_t strb = two_chromosomes ? sb : sa;
    std::vector<uint32_t> n11(na * nb), gg(na * nb), ca(na), heta(na), homa(na), cb(nb), hetb(nb), homb(nb);
    std::vector<uint32_t> w11(na * nb, 0), wgg(na * nb, 0), wca(na, 0), wheta(na, 0), whoma(na, 0), wcb(nb, 0), whetb(nb, 0), whomb(nb, 0);
    for (size_t i = i0; i < i0 + ni; i++) {
        for (size_t j = 0; j < na; j++) { const unsigned g = hap(A, sa, 2 * i, a0 + j) + hap(A, sa, 2 * i + 1, a0 + j); wca[j] += g; wheta[j] += g == 1; whoma[j] += g == 2; }
        for (size_t k = 0; k < nb; k++) { const unsigned g = hap(B, strb, 2 * i, b0 + k) + hap(B, strb, 2 * i + 1, b0 + k); wcb[k] += g; whetb[k] += g == 1; whomb[k] += g == 2; }
        for (size_t j = 0; j < na; j++)
            for (size_t k = 0; k < nb; k++) {
                const unsigned a_0 = hap(A, sa, 2 * i, a0 + j), a_1 = hap(A, sa, 2 * i + 1, a0 + j), b_0 = hap(B, strb, 2 * i, b0 + k), b_1 = hap(B, strb, 2 * i + 1, b0 + k);
                w11[j * nb + k] += a_0 * b_0 + a_1 * b_1; wgg[j * nb + k] += (a_0 + a_1) * (b_0 + b_1);
            }
    }
    gev_ld_counts_host(A.data(), sa, a0, na, B.data(), strb, b0, nb, i0, ni, n11.data(), gg.data(), ca.data(), heta.data(), homa.data(), cb.data(), hetb.data(), homb.data());
    n_checked++;
    if (n11 != w11 || gg != wgg || ca != wca || heta != wheta || homa != whoma || cb != wcb || hetb != whetb || homb != whomb) {
        n_bad++;
        printf("MISMATCH: block a [%zu,+%zu) of %zu, b [%zu,+%zu) of %zu%s, individuals [%zu,+%zu), stride + %zu\n", a0, na, La, b0, nb, Lb, two_chromosomes ? " (another chromosome)" : "", i0, ni, extra);
    }
}

// the quantum by long double arithmetic on the exact integers: the double route may differ from it by its three roundings only
static void check_scores(size_t L, size_t extra, size_t s0, size_t ns, size_t w, size_t i0, size_t ni, bool genotype)
{
    const size_t stride = (L + 63) / 64 + extra;
    std::vector<uint32_t> lo(ns), hi(ns);
    for (size_t t = 0; t < ns; t++) { const size_t j = s0 + t; lo[t] = (uint32_t)(j > w ? j - w : 0); hi[t] = (uint32_t)std::min(j + w + 1, L); }
    const std::vector<uint64_t> R = make_rows(i0 + ni, L, stride, ns ? (hi[ns - 1] - 1) / 64 : 0);
    std::vector<uint64_t> score(ns); std::vector<uint32_t> terms(ns);
    gev_ld_scores_host(R.data(), stride, s0, ns, lo.data(), hi.data(), i0, ni, genotype, score.data(), terms.data());
    bool bad = false;
    const uint64_t N = ni, n = genotype ? N : 2 * N;
    auto stats = [&](size_t j, uint64_t& s, uint64_t& s2) {
        s = s2 = 0;
        for (size_t i = i0; i < i0 + ni; i++) {
            const unsigned a = hap(R, stride, 2 * i, j), b = hap(R, stride, 2 * i + 1, j);
            if (genotype) { s += a + b; s2 += (a + b) * (a + b); } else { s += a + b; s2 += a + b; }
        }
    };
    for (size_t t = 0; t < ns; t++) {
        uint64_t sj, sj2; stats(s0 + t, sj, sj2);
        const uint64_t den_j = n * sj2 - sj * sj;
        uint64_t want = 0; uint32_t want_terms = 0;
        for (size_t k = lo[t]; k < hi[t]; k++) {
            uint64_t sk, sk2; stats(k, sk, sk2);
            const uint64_t den_k = n * sk2 - sk * sk;
            want_terms += den_k != 0;
            den_k ? n_poly++ : n_mono++;
            if (!den_j || !den_k) continue;
            uint64_t prod = 0;
            for (size_t i = i0; i < i0 + ni; i++) {
                const unsigned a0 = hap(R, stride, 2 * i, s0 + t), a1 = hap(R, stride, 2 * i + 1, s0 + t), b0 = hap(R, stride, 2 * i, k), b1 = hap(R, stride, 2 * i + 1, k);
                prod += genotype ? (a0 + a1) * (b0 + b1) : a0 * b0 + a1 * b1;
            }
            const long double num = (long double)(int64_t)(n * prod) - (long double)(sj * sk);
            const long double q = num * num / ((long double)den_j * (long double)den_k) * 1099511627776.0L;
            const uint64_t got_q = gev_ld_r2_q40((int64_t)(n * prod) - (int64_t)(sj * sk), den_j, den_k);
            if (fabsl((long double)got_q - q) > 0.5L + q * 8.8817841970012523e-16L) bad = true;
            if (got_q != 0 && got_q != (1ull << 40)) n_between++;
            want += got_q;
        }
        if (score[t] != want || terms[t] != want_terms) bad = true;
    }
    n_checked++;
    if (bad) { n_bad++; printf("MISMATCH: scores of SNPs [%zu,+%zu) of %zu, w = %zu, individuals [%zu,+%zu), %s r2, stride + %zu\n", s0, ns, L, w, i0, ni, genotype ? "genotype" : "haplotype", extra); }
}

int main()
{
    const size_t n_people = 70, L = 200, Lb = 77;
    const size_t n_inds[] = {1, 2, 15, 16, 17, 31, 32, 33, 70};
    const size_t blocks[][4] = {{190, 1, 0, 1}, {0, 16, 0, 16}, {0, 15, 100, 17}, {10, 33, 30, 33}, {3, 129, 60, 33}, {0, 17, 5, 129}, {40, 129, 40, 129}, {199, 1, 0, 200}};
    const size_t cross[][4] = {{0, 33, 0, 77}, {150, 17, 60, 17}, {199, 1, 76, 1}};
    for (size_t ni : n_inds) {
        const size_t starts[] = {0, std::min<size_t>(5, n_people - ni), std::min<size_t>(37, n_people - ni), n_people - ni};
        for (size_t i0 : starts)
            for (size_t extra = 0; extra <= 3; extra += 3) {
                for (auto& b : blocks) check_block(L, L, extra, b[0], b[1], b[2], b[3], i0, ni, false);
                for (auto& b : cross) check_block(L, Lb, extra, b[0], b[1], b[2], b[3], i0, ni, true);
                check_block(L, L, extra, 10, 0, 20, 5, i0, ni, false); check_block(L, L, extra, 10, 4, 200, 0, i0, ni, false);
            }
        for (int genotype = 0; genotype < 2; genotype++)
            for (size_t w : {(size_t)0, (size_t)1, (size_t)50, L}) {
                check_scores(L, 3, 0, L, w, std::min<size_t>(5, n_people - ni), ni, genotype != 0);
                check_scores(L, 0, 60, 75, w, n_people - ni, ni, genotype != 0);
                check_scores(L, 0, 199, 1, w, 0, ni, genotype != 0);
            }
    }
    check_block(L, L, 0, 0, 16, 0, 16, 7, 0, false);                 // no individual: zeros
    // the quantum at its extremes
    {
        const uint64_t big = 1ull << 62;
        n_checked++;
        if (gev_ld_r2_q40(0, 1, 1) != 0 || gev_ld_r2_q40(1, 1, 1) != 1ull << 40 || gev_ld_r2_q40(-1, 1, 1) != 1ull << 40 || gev_ld_r2_q40((int64_t)big, big, big) != 1ull << 40 ||
            gev_ld_r2_q40(-(int64_t)big, big, big) != 1ull << 40 || gev_ld_r2_q40(5, 0, 7) != 0 || gev_ld_r2_q40(5, 7, 0) != 0 || gev_ld_r2_q40(1, big, big) != 0 ||
            gev_ld_r2_q40(3, 9, 2) != 1ull << 39 || gev_ld_r2_q40(1, 3, 1) != 366503875925ull) { n_bad++; printf("MISMATCH: the quantum's extremes\n"); }
    }
    if (!n_mono || !n_poly || !n_between) { n_bad++; printf("MISMATCH: the inputs hold %llu monomorphic and %llu polymorphic window SNPs, %llu quanta strictly between 0 and 2^40\n", n_mono, n_poly, n_between); }
    printf("%llu shapes checked, %llu mismatches\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
