// fmt_g_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_fmt_g.h against the C library's snprintf("%g"), host only.
// Build with sanitizers:  g++ -O1 -g -std=c++14 -fsanitize=address,undefined -fno-sanitize-recover=all tools/fmt_g_check.cpp -o fmt_g_check
// Every value is formatted twice: by the fast path with its fallback, and with the exact path forced.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../geneevolve_amd/csrc/gev_fmt_g.h"

static unsigned long long n_checked = 0, n_exact = 0, n_bad = 0;
static const GevFmtTables* T;

static void to_chars(const GevG& g, char* s) { memcpy(s, &g.lo, 8); memcpy(s + 8, &g.hi, 8); s[16] = 0; }
static void check(double v)
{
    char want[64], got[17];
    const int nw = snprintf(want, sizeof want, "%g", v);
    for (int forced = 0; forced < 2; forced++) {
        GevG g; uint32_t ex = 0;
        const uint32_t n = forced ? gev_fmt_g<true>(T, v, g, &ex) : gev_fmt_g<false>(T, v, g, &ex);
        to_chars(g, got);
        if ((int)n != nw || strcmp(want, got) != 0 || n > GEV_FMT_MAX) {
            if (n_bad++ < 20) printf("MISMATCH %a: snprintf \"%s\", header \"%s\" (%u bytes, exact path %s)\n", v, want, got, n, forced ? "forced" : (ex ? "taken" : "not taken"));
        }
        if (!forced) n_exact += ex;
    }
    n_checked++;
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

int main()
{
    T = &gev_fmt_host_tables();
    const double edge[] = {0.0, -0.0, 1, 0.1, 100000, 999999, 999999.5, 999999.4999999999, 1e6, 1000005, 1000015, 100000.5, 100001.5, 10000.25, 10000.75,
                           1000.125, 1000.375, 1e-4, 1e-5, 9.999995e-05, 9.9999949999e-05, 5e-324, DBL_MIN, DBL_MAX, INFINITY, -INFINITY, NAN, -NAN,
                           1e22, 1e23, 1e100, 123456789, -1.5, 2.5e-310, 0.3, 1.0 / 3};
    for (double v : edge) { check(v); check(-v); }
    // every power of two and of ten, with their neighbours
    for (int e = -1074; e <= 1023; e++) { const double v = ldexp(1.0, e); check(v); check(nextafter(v, 0)); check(nextafter(v, INFINITY)); }
    for (int k = -323; k <= 308; k++) { char s[32]; snprintf(s, sizeof s, "1e%d", k); const double v = strtod(s, nullptr); check(v); check(nextafter(v, 0)); check(nextafter(v, INFINITY)); }
    // random bit patterns
    for (int i = 0; i < (1 << 20); i++) { const uint64_t b = rng(); double v; memcpy(&v, &b, 8); check(v); }
    // random values of ordinary size
    for (int i = 0; i < (1 << 18); i++) check(((double)(int64_t)rng() / 9.223372036854775808e18) * 4.0);
    // the doubles nearest (d + 1/2) * 10^k, d of six digits: what a table cannot decide
    const unsigned long long before = n_exact;
    for (int i = 0; i < (1 << 17); i++) {
        const unsigned d = 100000u + (unsigned)(rng() % 900000u); const int k = -328 + (int)(rng() % 632u);
        char s[40]; snprintf(s, sizeof s, "%u5e%d", d, k - 1);
        const double v = strtod(s, nullptr);
        check(v); check(nextafter(v, 0)); check(nextafter(v, INFINITY));
    }
    printf("%llu values checked twice, %llu mismatches, exact path taken by %llu (%llu of them in the near-midpoint set)\n", n_checked, n_bad, n_exact, n_exact - before);
    if (n_exact == before) { printf("the near-midpoint set never took the exact path\n"); return 1; }
    return n_bad ? 1 : 0;
}
