// ibd_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_ibd.h (the two-cursor IBD walk, the base pairs by root population)
// against a per-position raster, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/ibd_check.cpp -o ibd_check
// Rows of 0 to 24 parts over a few labels on positions [base, base + 240), base = 0, 5 and 2^63 - 100: parts that tile the span, gaps,
// one-bp parts, adjacent parts with the same label, the same hap_index under two root populations; all pairs of 40 rows, square and
// rectangular, min_bp of 0, 1, 7, an occurring segment length and that plus one, each output null in turn.  The truth labels every
// position of every row and takes the runs of equal labels position by position.  Every buffer is exactly sized (parts: the sum of the
// rows' lengths, offsets: rows + 1, outputs: n_a * n_b), so a stray access is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../geneevolve_amd/csrc/gev_ibd.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static unsigned long long n_checked = 0, n_bad = 0, n_none = 0, n_multi = 0, n_adjacent = 0;
static const uint64_t SPAN = 240;

struct Lists { std::vector<gev_part> parts; std::vector<uint64_t> off; };

static Lists make_lists(size_t n_rows, uint64_t base)
{
    Lists l; l.off.push_back(0);
    for (size_t r = 0; r < n_rows; r++) {
        const unsigned k = r % 9 == 0 ? 0 : (unsigned)(rng() % 25);
        std::vector<uint64_t> cuts;
        for (unsigned q = 0; q + 1 < k; q++) cuts.push_back(1 + rng() % (SPAN - 1));
        cuts.push_back(0); cuts.push_back(SPAN);
        for (size_t i = 0; i < cuts.size(); i++) for (size_t j = i + 1; j < cuts.size(); j++) if (cuts[j] < cuts[i]) { uint64_t t = cuts[i]; cuts[i] = cuts[j]; cuts[j] = t; }
        for (unsigned q = 0; q < k; q++) {
            uint64_t st = cuts[q], en = cuts[q + 1];
            if (en > st + 1 && rng() % 8 == 0) en -= 1 + rng() % (en - st - 1);          // a gap behind the part
            gev_part p; p.st = base + st; p.en = base + en; p.hap_index = rng() % 3 + (rng() % 16 == 0 ? (1ull << 40) : 0); p.root_population = (int32_t)(rng() % 2); p.reserved = 0;
            if (!l.parts.empty() && l.off.back() < l.parts.size() && rng() % 4 == 0) { p.hap_index = l.parts.back().hap_index; p.root_population = l.parts.back().root_population; }
            if (l.off.back() < l.parts.size() && l.parts.back().en == p.st && l.parts.back().hap_index == p.hap_index && l.parts.back().root_population == p.root_population) n_adjacent++;
            l.parts.push_back(p);
        }
        l.off.push_back(l.parts.size());
    }
    l.parts.shrink_to_fit();
    return l;
}
// label id of every position of every row: 0 = not covered, else 1 + an index of (root_population, hap_index)
static std::vector<uint64_t> rasterise(const Lists& l, uint64_t base)
{
    const size_t rows = l.off.size() - 1;
    std::vector<uint64_t> lab(rows * SPAN, 0);
    for (size_t r = 0; r < rows; r++)
        for (uint64_t q = l.off[r]; q < l.off[r + 1]; q++)
            for (uint64_t x = l.parts[q].st; x < l.parts[q].en; x++)
                lab[r * SPAN + (x - base)] = 1 + (uint64_t)l.parts[q].root_population + 2 * (l.parts[q].hap_index & 0xff) + 512 * (l.parts[q].hap_index >> 40);
    return lab;
}
static void check(const Lists& A, const Lists& B, uint64_t base, uint64_t min_bp, int null_out, bool count)
{
    const size_t na = A.off.size() - 1, nb = B.off.size() - 1;
    const std::vector<uint64_t> la = rasterise(A, base), lb = rasterise(B, base);
    std::vector<uint64_t> sh(null_out == 0 ? 0 : na * nb), mx(null_out == 2 ? 0 : na * nb); std::vector<uint32_t> ns(null_out == 1 ? 0 : na * nb);
    gev_ibd_host(A.parts.data(), A.off.data(), na, B.parts.data(), B.off.data(), nb, min_bp, null_out == 0 ? nullptr : sh.data(), null_out == 1 ? nullptr : ns.data(), null_out == 2 ? nullptr : mx.data());
    bool bad = false;
    for (size_t a = 0; a < na; a++)
        for (size_t b = 0; b < nb; b++) {
            uint64_t w_sh = 0, w_mx = 0, run = 0; uint32_t w_ns = 0;
            for (uint64_t x = 0; x <= SPAN; x++) {
                if (x < SPAN && la[a * SPAN + x] && la[a * SPAN + x] == lb[b * SPAN + x]) { run++; continue; }
                if (run >= min_bp && run) { w_sh += run; w_ns++; if (run > w_mx) w_mx = run; }
                run = 0;
            }
            if (count) { n_none += w_ns == 0; n_multi += w_ns >= 2; }
            if ((null_out != 0 && sh[a * nb + b] != w_sh) || (null_out != 1 && ns[a * nb + b] != w_ns) || (null_out != 2 && mx[a * nb + b] != w_mx)) bad = true;
        }
    n_checked++;
    if (bad) { n_bad++; printf("MISMATCH: %zu x %zu rows at base %llu, min_bp %llu, output %d null\n", na, nb, (unsigned long long)base, (unsigned long long)min_bp, null_out); }
}
static void check_ancestry(const Lists& A, uint64_t base)
{
    const std::vector<uint64_t> la = rasterise(A, base);
    bool bad = false;
    for (size_t r = 0; r + 1 < A.off.size(); r++) {
        uint64_t want[2] = {0, 0}, got[2] = {77, 77};
        for (uint64_t x = 0; x < SPAN; x++) if (la[r * SPAN + x]) want[(la[r * SPAN + x] - 1) & 1]++;
        const uint32_t n = (uint32_t)(A.off[r + 1] - A.off[r]);
        if (!gev_ancestry_row(n ? A.parts.data() + A.off[r] : nullptr, n, 2, got) || got[0] != want[0] || got[1] != want[1]) bad = true;
        uint64_t one[1] = {77};
        bool any1 = false;
        for (uint64_t q = A.off[r]; q < A.off[r + 1]; q++) any1 = any1 || A.parts[q].root_population == 1;
        if (gev_ancestry_row(n ? A.parts.data() + A.off[r] : nullptr, n, 1, one) == any1 || (any1 && one[0] != 77)) bad = true;       // a root population beyond n_pop: refused, nothing written
    }
    n_checked++;
    if (bad) { n_bad++; printf("MISMATCH: base pairs by root population at base %llu\n", (unsigned long long)base); }
}

int main()
{
    const uint64_t bases[] = {0, 5, (1ull << 63) - 100};
    for (uint64_t base : bases) {
        const Lists A = make_lists(40, base), B = make_lists(13, base), none = make_lists(0, base);
        check(A, A, base, 0, -1, true);
        check(A, B, base, 0, -1, false); check(B, A, base, 0, -1, false);
        check(A, none, base, 0, -1, false); check(none, B, base, 0, -1, false);
        // an occurring segment length: the longest of pair (1, 2)
        uint64_t mx = 0;
        { const Lists one = {std::vector<gev_part>(A.parts.begin() + A.off[1], A.parts.begin() + A.off[3]), {0, A.off[2] - A.off[1], A.off[3] - A.off[1]}};
          uint64_t m[4]; gev_ibd_host(one.parts.data(), one.off.data(), 2, one.parts.data(), one.off.data(), 2, 0, nullptr, nullptr, m); mx = m[1]; }
        for (uint64_t min_bp : {(uint64_t)1, (uint64_t)7, mx, mx + 1, ~(uint64_t)0}) { check(A, A, base, min_bp, -1, false); check(A, B, base, min_bp, -1, false); }
        for (int null_out = 0; null_out < 3; null_out++) check(A, B, base, 3, null_out, false);
        check_ancestry(A, base);
    }
    if (!n_none || !n_multi || !n_adjacent) { n_bad++; printf("MISMATCH: the inputs hold %llu pairs that share nothing, %llu with several segments, %llu adjacent parts with one label\n", n_none, n_multi, n_adjacent); }
    printf("%llu shapes checked, %llu mismatches (%llu pairs share nothing, %llu have several segments, %llu adjacent same-label parts)\n", n_checked, n_bad, n_none, n_multi, n_adjacent);
    return n_bad ? 1 : 0;
}
