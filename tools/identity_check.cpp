// identity_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_identity.h (the four-cursor walk over the lists of two individuals,
// Jacquard's nine identity states) against a per-position truth, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/identity_check.cpp -o identity_check
// Rows of 0 to 24 parts over a few labels on positions [base, base + 240), base = 0, 5 and 2^63 - 100: parts that tile the span, gaps,
// one-bp parts, zero-length and inverted parts, adjacent parts with the same label, the same hap_index under two root populations, a
// hap_index beyond 2^32; all pairs of 20 individuals, square and rectangular, a side without individuals.  The truth labels every position
// of every row, writes the four labels of a pair at a position as a restricted-growth string and looks it up in a literal table.  Every
// buffer is exactly sized (parts: the sum of the rows' lengths, offsets: 2 n + 1, planes: 9 n_a n_b), so a stray access is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../geneevolve_amd/csrc/gev_identity.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static unsigned long long n_checked = 0, n_bad = 0, n_empty_parts = 0, n_adjacent = 0, in_state[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
static const uint64_t SPAN = 240;
static const struct { const char* rgs; int state; } TABLE[15] = {
    {"0000", 1}, {"0011", 2}, {"0001", 3}, {"0010", 3}, {"0012", 4}, {"0100", 5}, {"0111", 5}, {"0122", 6},
    {"0101", 7}, {"0110", 7}, {"0102", 8}, {"0120", 8}, {"0112", 8}, {"0121", 8}, {"0123", 9}};

struct Lists { std::vector<gev_part> parts; std::vector<uint64_t> off; };

static Lists make_lists(size_t n_ind, uint64_t base)
{
    Lists l; l.off.push_back(0);
    for (size_t r = 0; r < 2 * n_ind; r++) {
        const unsigned k = r % 13 == 5 ? 0 : (unsigned)(rng() % 25);
        std::vector<uint64_t> cuts;
        for (unsigned q = 0; q + 1 < k; q++) cuts.push_back(1 + rng() % (SPAN - 1));
        cuts.push_back(0); cuts.push_back(SPAN);
        for (size_t i = 0; i < cuts.size(); i++) for (size_t j = i + 1; j < cuts.size(); j++) if (cuts[j] < cuts[i]) { uint64_t t = cuts[i]; cuts[i] = cuts[j]; cuts[j] = t; }
        for (unsigned q = 0; q < k; q++) {
            uint64_t st = cuts[q], en = cuts[q + 1];
            if (en > st + 1 && rng() % 8 == 0) en -= 1 + rng() % (en - st - 1);          // a gap behind the part
            gev_part p; p.st = base + st; p.en = base + en; p.hap_index = rng() % 3 + (rng() % 16 == 0 ? (1ull << 40) : 0); p.root_population = (int32_t)(rng() % 2); p.reserved = 0;
            if (l.off.back() < l.parts.size() && rng() % 3 == 0) { p.hap_index = l.parts.back().hap_index; p.root_population = l.parts.back().root_population; }
            if (l.off.back() < l.parts.size() && l.parts.back().en == p.st && p.st < p.en && l.parts.back().hap_index == p.hap_index && l.parts.back().root_population == p.root_population) n_adjacent++;
            if (rng() % 10 == 0) {                                                       // a part that covers nothing in front: zero-length, or inverted where st and en still do not decrease
                gev_part z = p; z.hap_index = 7; z.en = z.st;
                if (st > 0 && rng() % 2 == 0 && l.off.back() < l.parts.size() && l.parts.back().en < z.st) z.en = z.st - 1;
                l.parts.push_back(z); n_empty_parts++;
            }
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
static int state_of(const uint64_t four[4])
{
    char rgs[5] = {0, 0, 0, 0, 0};
    uint64_t seen[4]; int n_seen = 0;
    for (int h = 0; h < 4; h++) {
        int at = 0;
        while (at < n_seen && seen[at] != four[h]) at++;
        if (at == n_seen) seen[n_seen++] = four[h];
        rgs[h] = (char)('0' + at);
    }
    for (const auto& t : TABLE) if (!strcmp(t.rgs, rgs)) return t.state;
    return 0;
}
static void check(const Lists& A, const Lists& B, uint64_t base, bool count)
{
    const size_t na = (A.off.size() - 1) / 2, nb = (B.off.size() - 1) / 2;
    const std::vector<uint64_t> la = rasterise(A, base), lb = rasterise(B, base);
    std::vector<uint64_t> bp(9 * na * nb);
    for (auto& x : bp) x = 0x7777;
    gev_identity_host(A.parts.data(), A.off.data(), na, B.parts.data(), B.off.data(), nb, bp.data());
    bool bad = false;
    for (size_t i = 0; i < na; i++)
        for (size_t k = 0; k < nb; k++) {
            uint64_t want[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (uint64_t x = 0; x < SPAN; x++) {
                const uint64_t four[4] = {la[2 * i * SPAN + x], la[(2 * i + 1) * SPAN + x], lb[2 * k * SPAN + x], lb[(2 * k + 1) * SPAN + x]};
                if (!four[0] || !four[1] || !four[2] || !four[3]) continue;
                const int s = state_of(four);
                if (!s) { bad = true; continue; }
                want[s - 1]++;
            }
            for (size_t q = 0; q < 9; q++) {
                if (bp[(q * na + i) * nb + k] != want[q]) bad = true;
                if (count) in_state[q] += want[q] != 0;
            }
        }
    n_checked++;
    if (bad) { n_bad++; printf("MISMATCH: %zu x %zu individuals at base %llu\n", na, nb, (unsigned long long)base); }
}

int main()
{
    const uint64_t bases[] = {0, 5, (1ull << 63) - 100};
    for (uint64_t base : bases) {
        const Lists A = make_lists(20, base), B = make_lists(7, base), none = make_lists(0, base);
        check(A, A, base, true);
        check(A, B, base, false); check(B, A, base, false);
        check(A, none, base, false); check(none, B, base, false); check(none, none, base, false);
    }
    bool all_states = true;
    for (int q = 0; q < 9; q++) all_states = all_states && in_state[q];
    if (!all_states || !n_empty_parts || !n_adjacent) { n_bad++; printf("MISMATCH: the inputs miss a state, or hold %llu parts that cover nothing and %llu adjacent parts with one label\n", n_empty_parts, n_adjacent); }
    printf("%llu shapes checked, %llu mismatches (pairs with base pairs in D1 .. D9:", n_checked, n_bad);
    for (int q = 0; q < 9; q++) printf(" %llu", in_state[q]);
    printf("; %llu parts that cover nothing, %llu adjacent same-label parts)\n", n_empty_parts, n_adjacent);
    return n_bad ? 1 : 0;
}
