// lineage_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_lineage.h (the cursor walk over sorted positions, the label check, the
// site reductions and their merge) against a per-position raster, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/lineage_check.cpp -o lineage_check
// Rows of 0 to 24 parts over the founders of three root populations (one of them without founders) on positions [base, base + 240),
// base = 0, 5 and 2^63 - 100: parts that tile the span, gaps, one-bp parts, zero-length and inverted parts that keep st and en from
// decreasing, the same hap_index under two root populations.  Positions: all of [base - 2, base + 242) that exist, with duplicates, and
// thinned sets (a cursor then passes over several parts at once); 40 rows, 13 rows, no rows, no positions; each output null in turn.  The
// truth labels every position of every row by its covering part and counts per position.  A site record is also rebuilt from partial
// records over founder tiles of 5 merged in both orders (what the device's tiles do).  Every buffer is exactly sized (parts: the sum of
// the rows' lengths, offsets: rows + 1, fid: n_pos * n_rows, counts: n_pos * F, site: n_pos, pop_counts: n_pos * n_pop), so a stray
// access is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../geneevolve_amd/csrc/gev_lineage.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static unsigned long long n_checked = 0, n_bad = 0, n_uncovered = 0, n_ties = 0, n_unique = 0, n_empty_parts = 0, n_tile_merges = 0;
static const uint64_t SPAN = 240;
static const int N_POP = 3;
static const uint64_t NFH[N_POP] = {7, 0, 6};                 // base 0, 7, 7; F = 13
static const uint64_t BASE[N_POP + 1] = {0, 7, 7, 13};

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
        uint64_t last_en = 0;
        for (unsigned q = 0; q < k; q++) {
            uint64_t st = cuts[q], en = cuts[q + 1];
            if (en > st + 1 && rng() % 8 == 0) en -= 1 + rng() % (en - st - 1);          // a gap behind the part
            if (en > st && st > last_en && rng() % 16 == 0) { const uint64_t t = st; st = en; en = t; }    // inverted: st and en still do not decrease along the row
            gev_part p; p.st = base + st; p.en = base + en; p.root_population = rng() % 2 ? 2 : 0; p.hap_index = rng() % NFH[p.root_population]; p.reserved = 0;
            if (p.st >= p.en) n_empty_parts++;
            if (en > last_en) last_en = en;
            l.parts.push_back(p);
        }
        l.off.push_back(l.parts.size());
    }
    l.parts.shrink_to_fit();
    return l;
}
static bool same_site(const gev_lineage_site& a, const gev_lineage_site& b)
{
    return a.sum_sq == b.sum_sq && a.n_covered == b.n_covered && a.n_lineages == b.n_lineages && a.top_count == b.top_count && a.top_founder == b.top_founder;
}
// null_out: 0 fid, 1 counts, 2 site, 3 pop_counts, -1 none
static void check(const Lists& A, const std::vector<uint64_t>& pos, int null_out, bool count)
{
    const size_t n_rows = A.off.size() - 1, n_pos = pos.size(), F = (size_t)BASE[N_POP];
    std::vector<uint32_t> fid(null_out == 0 ? 0 : n_pos * n_rows), counts(null_out == 1 ? 0 : n_pos * F), pc(null_out == 3 ? 0 : n_pos * N_POP);
    std::vector<gev_lineage_site> site(null_out == 2 ? 0 : n_pos);
    uint32_t bad_labels = 0;
    for (size_t r = 0; r < n_rows; r++) bad_labels |= gev_lineage_check_row(A.parts.data() + A.off[r], (uint32_t)(A.off[r + 1] - A.off[r]), NFH, N_POP);
    gev_lineage_host(A.parts.data(), A.off.data(), n_rows, pos.data(), n_pos, BASE, N_POP, null_out == 0 ? nullptr : fid.data(), null_out == 1 ? nullptr : counts.data(),
                     null_out == 2 ? nullptr : site.data(), null_out == 3 ? nullptr : pc.data());
    bool bad = bad_labels != 0;
    for (size_t p = 0; p < n_pos; p++) {
        std::vector<uint32_t> w_cnt(F, 0), w_pc(N_POP, 0);
        for (size_t r = 0; r < n_rows; r++) {
            uint32_t w = GEV_NO_FOUNDER;
            for (uint64_t q = A.off[r]; q < A.off[r + 1]; q++)
                if (A.parts[q].st <= pos[p] && pos[p] < A.parts[q].en) { w = (uint32_t)(BASE[A.parts[q].root_population] + A.parts[q].hap_index); w_pc[A.parts[q].root_population]++; }
            if (w != GEV_NO_FOUNDER) w_cnt[w]++;
            if (null_out != 0 && fid[p * n_rows + r] != w) bad = true;
        }
        gev_lineage_site w; w.sum_sq = 0; w.n_covered = 0; w.n_lineages = 0; w.top_count = 0; w.top_founder = GEV_NO_FOUNDER;
        unsigned at_top = 0;
        for (size_t f = 0; f < F; f++) {
            w.sum_sq += (uint64_t)w_cnt[f] * w_cnt[f]; w.n_covered += w_cnt[f]; w.n_lineages += w_cnt[f] != 0;
            if (w_cnt[f] > w.top_count) { w.top_count = w_cnt[f]; w.top_founder = (uint32_t)f; at_top = 1; } else if (w_cnt[f] && w_cnt[f] == w.top_count) at_top++;
        }
        if (count) { n_uncovered += w.n_covered == 0; n_ties += at_top >= 2; n_unique += at_top == 1; }
        if (null_out != 1) for (size_t f = 0; f < F; f++) if (counts[p * F + f] != w_cnt[f]) bad = true;
        if (null_out != 2 && !same_site(site[p], w)) bad = true;
        if (null_out != 3) for (int q = 0; q < N_POP; q++) if (pc[p * N_POP + q] != w_pc[q]) bad = true;
        // the record from partial records over tiles of 5 founders, merged in ascending and in descending tile order
        for (int dir = 0; dir < 2; dir++) {
            gev_lineage_site m = gev_lineage_empty();
            const size_t n_tiles = (F + 4) / 5;
            for (size_t k = 0; k < n_tiles; k++) {
                const size_t tile = dir ? n_tiles - 1 - k : k;
                gev_lineage_site t = gev_lineage_empty();
                for (size_t f = 5 * tile + 5 < F ? 5 * tile + 5 : F; f-- > 5 * tile;) gev_lineage_add(t, (uint32_t)f, w_cnt[f]);       // (descending inside the tile)
                gev_lineage_merge(m, t);
            }
            n_tile_merges++;
            if (!same_site(m, w)) bad = true;
        }
    }
    n_checked++;
    if (bad) { n_bad++; printf("MISMATCH: %zu rows, %zu positions from %llu, output %d null\n", n_rows, n_pos, n_pos ? (unsigned long long)pos[0] : 0ull, null_out); }
}
// a bad label is found whichever part carries it, and nothing else is
static void check_labels(const Lists& A)
{
    bool bad = false;
    for (size_t r = 0; r + 1 < A.off.size(); r++) {
        const uint32_t n = (uint32_t)(A.off[r + 1] - A.off[r]);
        if (!n) continue;
        std::vector<gev_part> row(A.parts.begin() + A.off[r], A.parts.begin() + A.off[r + 1]);
        if (gev_lineage_check_row(row.data(), n, NFH, N_POP)) bad = true;
        const uint32_t q = (uint32_t)(rng() % n);
        gev_part keep = row[q];
        row[q].hap_index = NFH[row[q].root_population];
        if (gev_lineage_check_row(row.data(), n, NFH, N_POP) != GEV_LINEAGE_BAD_HAP) bad = true;
        row[q] = keep; row[q].root_population = 1; row[q].hap_index = 0;                       // a root population without founders
        if (gev_lineage_check_row(row.data(), n, NFH, N_POP) != GEV_LINEAGE_BAD_HAP) bad = true;
        row[q].root_population = rng() % 2 ? N_POP : -1;
        if (gev_lineage_check_row(row.data(), n, NFH, N_POP) != GEV_LINEAGE_BAD_POP) bad = true;
    }
    n_checked++;
    if (bad) { n_bad++; printf("MISMATCH: the label check\n"); }
}

int main()
{
    const uint64_t bases[] = {0, 5, (1ull << 63) - 100};
    for (uint64_t base : bases) {
        const Lists A = make_lists(40, base), B = make_lists(13, base), none = make_lists(0, base);
        std::vector<uint64_t> all, thin, sparse, one(1, base + 17), empty;
        for (uint64_t x = base >= 2 ? base - 2 : 0; x < base + SPAN + 2; x++) { all.push_back(x); if (x % 7 == 3) all.push_back(x); if (x % 5 == 0) thin.push_back(x); if (x % 61 == 9) sparse.push_back(x); }
        all.shrink_to_fit(); thin.shrink_to_fit(); sparse.shrink_to_fit();
        check(A, all, -1, true);
        check(B, all, -1, false); check(A, thin, -1, false); check(A, sparse, -1, false); check(B, one, -1, false);
        check(none, all, -1, false); check(A, empty, -1, false); check(none, empty, -1, false);
        for (int null_out = 0; null_out < 4; null_out++) { check(A, thin, null_out, false); check(none, thin, null_out, false); }
        check_labels(A);
    }
    // the extremes of the position: a part that ends at 2^64 - 1 does not cover it
    {
        Lists l; gev_part p; p.st = ~0ull - 9; p.en = ~0ull; p.hap_index = 3; p.root_population = 2; p.reserved = 0;
        l.parts.push_back(p); l.off.push_back(0); l.off.push_back(1); l.parts.shrink_to_fit();
        std::vector<uint64_t> pos; pos.push_back(0); pos.push_back(~0ull - 10); pos.push_back(~0ull - 9); pos.push_back(~0ull - 1); pos.push_back(~0ull); pos.shrink_to_fit();
        check(l, pos, -1, false);
    }
    if (!n_uncovered || !n_ties || !n_unique || !n_empty_parts) { n_bad++; printf("MISMATCH: the inputs hold %llu uncovered positions, %llu ties for the top, %llu unique tops, %llu parts that cover nothing\n", n_uncovered, n_ties, n_unique, n_empty_parts); }
    printf("%llu shapes checked, %llu mismatches (%llu uncovered positions, %llu ties for the top, %llu unique tops, %llu parts that cover nothing, %llu merges over tiles)\n",
           n_checked, n_bad, n_uncovered, n_ties, n_unique, n_empty_parts, n_tile_merges);
    return n_bad ? 1 : 0;
}
