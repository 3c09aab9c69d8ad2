// roh_check.cpp -- stand-alone check of the runs-of-homozygosity word logic of geneevolve_amd/csrc/gev_roh.h (gev_roh_rows_host,
// gev_roh_cover_host, gev_roh_segments_fit_host) against a per-SNP loop, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/roh_check.cpp -o roh_check
// The shapes are those of tests/roh_inputs.py: L = 3 * 8192 + 77 SNPs; individuals that are all homozygous, all heterozygous, with a
// het at every multiple of 64, at bit 63 of every word, at SNP 0 and L - 1 alone, with a single het at B - 1, B and B + 1 of every edge
// B in {64, 128, 4096, 8192, 16384}, and with random hets at one SNP in 50, 500 and 5000; positions 100 bp apart with gaps of 5100 bp
// behind SNPs 0, 63, 64, 4095, 8191 and L - 2 and three columns at one position; no limits, min_snps and min_bp at an occurring length
// and one above, max_gap_bp of 0, at the gap and one below; SNP ranges of one SNP at both ends, across a word edge, beginning and
// ending inside words, the whole row; individual sub-ranges.  The truth walks SNP by SNP: a run goes on while the two rows agree and
// the gap rule holds.  Every shape runs the summary with the cover and the three calls of the capacity rule (count-only, a buffer of
// exactly n_total records, which must be filled, and one of n_total - 1, which must come back as it was).  Every buffer is exactly
// sized (rows of ceil(L / 64) words, L positions, n_snps + 1 differences, the records), so a stray access is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../geneevolve_amd/csrc/gev_roh.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static unsigned long long n_checked = 0, n_bad = 0, n_records = 0;
static const size_t L = 3 * 8192 + 77, W = (L + 63) / 64;

struct Truth { std::vector<uint32_t> n_roh, roh_snps, cover; std::vector<uint64_t> roh_bp, max_bp; std::vector<gev_roh_segment> rec; };

static bool bit(const uint64_t* row, size_t j) { return (row[j >> 6] >> (j & 63)) & 1u; }
static Truth truth(const uint64_t* bits, const uint64_t* pos, size_t s0, size_t ns, size_t i0, size_t ni, const gev_roh_params& q)
{
    Truth t;
    t.n_roh.assign(ni, 0); t.roh_snps.assign(ni, 0); t.roh_bp.assign(ni, 0); t.max_bp.assign(ni, 0); t.cover.assign(ns, 0);
    for (size_t i = 0; i < ni; i++) {
        const uint64_t *a = bits + 2 * (i0 + i) * W, *b = a + W;
        size_t j0 = 0; bool open = false;
        for (size_t j = s0; j <= s0 + ns; j++) {
            const bool hom = j < s0 + ns && bit(a, j) == bit(b, j);
            const bool goes_on = open && hom && !(q.max_gap_bp && pos[j] - pos[j - 1] > q.max_gap_bp);
            if (open && !goes_on) {
                const size_t j1 = j - 1, n = j1 - j0 + 1;
                if (n >= q.min_snps && pos[j1] - pos[j0] >= q.min_bp) {
                    t.n_roh[i]++; t.roh_snps[i] += (uint32_t)n; t.roh_bp[i] += pos[j1] - pos[j0];
                    if (pos[j1] - pos[j0] > t.max_bp[i]) t.max_bp[i] = pos[j1] - pos[j0];
                    for (size_t x = j0; x <= j1; x++) t.cover[x - s0]++;
                    gev_roh_segment r; r.st = pos[j0]; r.en = pos[j1]; r.ind = (uint32_t)(i0 + i); r.snp_first = (uint32_t)j0; r.n_snps = (uint32_t)n; r.reserved = 0;
                    t.rec.push_back(r);
                }
                open = false;
            }
            if (hom && !open) { open = true; j0 = j; }
        }
    }
    return t;
}
static bool same_record(const gev_roh_segment& x, const gev_roh_segment& y)
{
    return x.st == y.st && x.en == y.en && x.ind == y.ind && x.snp_first == y.snp_first && x.n_snps == y.n_snps && x.reserved == y.reserved;
}
static void check(const uint64_t* bits, const uint64_t* pos, size_t s0, size_t ns, size_t i0, size_t ni, const gev_roh_params& q)
{
    const Truth want = truth(bits, pos, s0, ns, i0, ni, q);
    bool bad = false;
    std::vector<uint32_t> n_roh(ni), roh_snps(ni), diff(ns + 1, 0), cover(ns);
    std::vector<uint64_t> roh_bp(ni), max_bp(ni);
    gev_roh_rows_host(bits, W, pos, L, s0, ns, i0, ni, q, n_roh.data(), roh_bp.data(), roh_snps.data(), max_bp.data(), diff.data(), nullptr);
    gev_roh_cover_host(diff.data(), ns, cover.data());
    if (n_roh != want.n_roh || roh_snps != want.roh_snps || roh_bp != want.roh_bp || max_bp != want.max_bp || cover != want.cover) bad = true;
    uint64_t total = ~(uint64_t)0;
    gev_roh_segments_fit_host(bits, W, pos, L, s0, ns, i0, ni, q, nullptr, 0, &total);                          // count-only
    if (total != want.rec.size()) bad = true;
    else {
        uint64_t again = ~(uint64_t)0;
        gev_roh_segment* out = (gev_roh_segment*)malloc(total * sizeof(gev_roh_segment) + (total == 0));      // capacity == n_total, exactly that many records: filled
        gev_roh_segments_fit_host(bits, W, pos, L, s0, ns, i0, ni, q, out, (size_t)total, &again);
        if (again != total) bad = true;
        for (size_t k = 0; k < total && !bad; k++) if (!same_record(out[k], want.rec[k])) bad = true;
        free(out);
        if (total) {                                                   // capacity == n_total - 1, exactly that many records: the total is right, nothing is written
            const size_t capacity = (size_t)total - 1, bytes = capacity * sizeof(gev_roh_segment);
            unsigned char* guard = (unsigned char*)malloc(bytes + (bytes == 0));
            memset(guard, 0xA5, bytes);
            again = ~(uint64_t)0;
            gev_roh_segments_fit_host(bits, W, pos, L, s0, ns, i0, ni, q, (gev_roh_segment*)guard, capacity, &again);
            if (again != total) bad = true;
            for (size_t k = 0; k < bytes; k++) if (guard[k] != 0xA5) bad = true;
            free(guard);
        }
    }
    n_checked++; n_records += total;
    if (bad) { n_bad++; printf("MISMATCH: SNPs [%zu,+%zu) individuals [%zu,+%zu) min_snps %u min_bp %llu max_gap_bp %llu: %llu records, %zu expected\n", s0, ns, i0, ni, q.min_snps,
                               (unsigned long long)q.min_bp, (unsigned long long)q.max_gap_bp, (unsigned long long)total, want.rec.size()); }
}

int main()
{
    // positions
    std::vector<uint64_t> pos(L);
    const size_t gaps_after[] = {0, 63, 64, 4095, 8191, L - 2};
    { uint64_t x = 1000;
      for (size_t j = 0; j < L; j++) {
          if (j) x += (j == 201 || j == 202) ? 0 : 100;
          for (size_t g : gaps_after) if (j == g + 1) x += 5000;
          pos[j] = x;
      } }
    // the individuals' het masks, then rows: a random, b = a ^ het
    std::vector<std::vector<bool>> het;
    het.push_back(std::vector<bool>(L, false));
    het.push_back(std::vector<bool>(L, true));
    { std::vector<bool> m(L, false); for (size_t j = 0; j < L; j += 64) m[j] = true; het.push_back(m); }
    { std::vector<bool> m(L, false); for (size_t j = 63; j < L; j += 64) m[j] = true; het.push_back(m); }
    { std::vector<bool> m(L, false); m[0] = m[L - 1] = true; het.push_back(m); }
    for (size_t edge : {(size_t)64, (size_t)128, (size_t)4096, (size_t)8192, (size_t)16384})
        for (size_t at = edge - 1; at <= edge + 1; at++) { std::vector<bool> m(L, false); m[at] = true; het.push_back(m); }
    for (unsigned k = 0; k < 9; k++) {
        const uint64_t one_in = k % 3 == 0 ? 50 : k % 3 == 1 ? 500 : 5000;
        std::vector<bool> m(L, false);
        for (size_t j = 0; j < L; j++) m[j] = rng() % one_in == 0;
        het.push_back(m);
    }
    const size_t n = het.size();
    std::vector<uint64_t> bits(2 * n * W, 0);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < L; j++) {
            const uint64_t a = rng() & 1u, b = a ^ (het[i][j] ? 1u : 0u);
            bits[2 * i * W + (j >> 6)] |= a << (j & 63); bits[(2 * i + 1) * W + (j >> 6)] |= b << (j & 63);
        }
    bits.shrink_to_fit();
    // an occurring run: the first of the first random individual
    const gev_roh_params none = {0, 0, 0, 0};
    const Truth all = truth(bits.data(), pos.data(), 0, L, 0, n, none);
    uint32_t n0 = 0; uint64_t bp0 = 0;
    for (const gev_roh_segment& r : all.rec) if (r.ind == 20 && r.n_snps > 3) { n0 = r.n_snps; bp0 = r.en - r.st; break; }
    if (!n0 || all.n_roh[0] != 1 || all.roh_snps[0] != L || all.n_roh[1] != 0) { n_bad++; printf("MISMATCH: the inputs are not what the cases need\n"); }
    const gev_roh_params sets[] = {none, {n0, 0, 0, 0}, {n0 + 1, 0, 0, 0}, {0, 0, bp0, 0}, {0, 0, bp0 + 1, 0}, {0, 0, 0, 5100}, {0, 0, 0, 5099}, {n0, 0, bp0, 5099}};
    const size_t ranges[][2] = {{0, 1}, {L - 1, 1}, {60, 10}, {70, 50}, {37, 8192 + 100}, {8191, 2}, {4000, 16384 + 500}, {1, L - 1}, {0, L}, {L, 0}};
    for (const gev_roh_params& q : sets)
        for (const auto& r : ranges) check(bits.data(), pos.data(), r[0], r[1], 0, n, q);
    const size_t inds[][2] = {{0, 1}, {n - 1, 1}, {1, n - 2}, {5, 15}, {17, 0}};
    for (const auto& ind : inds) {
        check(bits.data(), pos.data(), 0, L, ind[0], ind[1], sets[7]);
        check(bits.data(), pos.data(), 37, 8292, ind[0], ind[1], sets[0]);
    }
    if (!n_records) { n_bad++; printf("MISMATCH: no records\n"); }
    printf("%llu shapes checked, %llu mismatches (%llu records)\n", n_checked, n_bad, n_records);
    return n_bad ? 1 : 0;
}
