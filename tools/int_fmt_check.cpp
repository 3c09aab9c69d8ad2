// int_fmt_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_fmt_int.h against snprintf("%llu") / std::to_string, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/int_fmt_check.cpp -o int_fmt_check
// Checks the split by 10^8, the digit count, the decimal of a u64 and of an int, and whole lines with their measured length.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../geneevolve_amd/csrc/gev_fmt_int.h"

static unsigned long long n_checked = 0, n_bad = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

static void check_u64(uint64_t v)
{
    char want[32];
    const int nw = snprintf(want, sizeof want, "%llu", (unsigned long long)v);
    std::vector<char> got(nw + 2, '#');                       // exactly sized, one guard byte on either side: a stray digit is a mismatch (or a sanitizer report)
    GevIntMemSink s{got.data() + 1};
    const uint32_t end = gev_int_dec(s, 0, v);
    const bool ok = (int)end == nw && (int)gev_int_dec_len(v) == nw && memcmp(got.data() + 1, want, nw) == 0 && got[0] == '#' && got[nw + 1] == '#'
                    && gev_int_div1e8(v) == v / 100000000ull;
    if (!ok && n_bad++ < 20) printf("MISMATCH %llu: header \"%.*s\" (%u digits)\n", (unsigned long long)v, (int)end, got.data() + 1, end);
    n_checked++;
}
static void check_int(int v)
{
    const std::string want = std::to_string(v);
    std::vector<char> got(want.size() + 2, '#');
    GevIntMemSink s{got.data() + 1};
    const uint32_t end = gev_int_sdec(s, 0, v);
    const bool ok = end == want.size() && gev_int_sdec_len(v) == want.size() && memcmp(got.data() + 1, want.data(), want.size()) == 0 && got[0] == '#' && got[want.size() + 1] == '#';
    if (!ok && n_bad++ < 20) printf("MISMATCH int %d\n", v);
    n_checked++;
}
static void check_line(const GevIntLine& l, const std::string& name)
{
    char want[256];
    const int nw = snprintf(want, sizeof want, "%llu %d %u %llu %llu %llu %s.%c %u\n", (unsigned long long)l.id1, l.chr_label, l.ihap, (unsigned long long)l.st, (unsigned long long)l.en,
                            (unsigned long long)l.hap1, name.c_str(), (l.hap1 & 1) ? '1' : '2', l.root1);
    std::vector<char> got(nw + 2, '#');
    GevIntMemSink s{got.data() + 1};
    const uint32_t len = gev_int_line_len(l, (uint32_t)name.size());
    bool ok = (int)len == nw && len <= GEV_INT_LINE_MAX;
    if (ok) ok = gev_int_line(s, 0, l, (const unsigned char*)name.data(), (uint32_t)name.size()) == len && memcmp(got.data() + 1, want, nw) == 0 && got[0] == '#' && got[nw + 1] == '#';
    if (!ok && n_bad++ < 20) printf("MISMATCH line: want \"%.*s\", measured %u bytes\n", nw - 1, want, len);
    n_checked++;
}

int main()
{
    // edges: 0, 9, 10, 10^k - 1, 10^k, 10^k + 1, the powers of two and their neighbours
    check_u64(0); check_u64(9); check_u64(UINT64_MAX); check_u64(INT64_MAX);
    uint64_t p = 1;
    for (int k = 0; k <= 19; k++) { check_u64(p - 1); check_u64(p); check_u64(p + 1); if (k < 19) p *= 10; }
    for (int b = 0; b < 64; b++) { const uint64_t v = 1ull << b; check_u64(v - 1); check_u64(v); check_u64(v + 1); }
    // multiples of 10^8 and of 10^16 and their neighbours: where the split by 10^8 could be one off
    for (int i = 0; i < (1 << 16); i++) {
        const uint64_t a = (rng() % 184467440737ull) * 100000000ull, b = (rng() % 1844ull) * 10000000000000000ull;
        check_u64(a); check_u64(a - 1); check_u64(a + 1); check_u64(b); check_u64(b - 1); check_u64(b + 1);
    }
    // random values of every length
    for (int i = 0; i < (1 << 22); i++) { const uint64_t v = rng(); check_u64(v >> (rng() & 63)); }
    const int ints[] = {0, 1, 9, 10, 22, 99, 100, 123, 999, 1000, 2147483647, -1, -9, -10, -2147483647 - 1};
    for (int v : ints) check_int(v);
    for (int i = 0; i < (1 << 16); i++) check_int((int)(uint32_t)rng());
    // whole lines
    const std::string names[] = {"a", "p0i1", std::string(GEV_INT_NAME_MAX, 'x')};
    check_line(GevIntLine{UINT64_MAX, UINT64_MAX, UINT64_MAX, UINT64_MAX, UINT32_MAX, 1u, -2147483647 - 1}, names[2]);    // the longest possible
    for (int i = 0; i < (1 << 18); i++) {
        GevIntLine l;
        l.id1 = rng() >> (rng() & 63); l.st = rng() >> (rng() & 63); l.en = rng() >> (rng() & 63); l.hap1 = rng() >> (rng() & 63);
        l.root1 = (uint32_t)rng() >> (rng() & 31); l.ihap = (uint32_t)(rng() & 1); l.chr_label = (int)((uint32_t)rng() >> (rng() & 31)) * ((rng() & 7) ? 1 : -1);
        check_line(l, names[rng() % 3]);
    }
    printf("%llu checks, %llu mismatches\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
