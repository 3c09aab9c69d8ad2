// info_format_host.cpp -- the host way to write a generation's .info rows, for tools/phenotype_loop_bench.py --info host: C snprintf on
// up to 8 threads, each formatting a contiguous slice of the individuals, the slices copied out in order.  This is what the bound
// command-line program does (integration/gev_glue.cpp, format_humans / save_human_info), on the arrays the library's downloads return.
// Build: g++ -O2 -std=c++14 -shared -fPIC -pthread tools/info_format_host.cpp -o tools/libinfo_format_host.so
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

static void format_rows(const int64_t* ids, const uint8_t* sex, const double* const* cols, int ncol, size_t i0, size_t i1, std::string& out)
{
    char buf[64];
    out.reserve((i1 - i0) * (64 + 13 * (size_t)ncol));
    for (size_t i = i0; i < i1; i++) {
        for (int f = 0; f < 7; f++) { const int n = snprintf(buf, sizeof buf, "%lu ", (unsigned long)(ids[i * 7 + f] + 1)); out.append(buf, (size_t)n); }
        { const int n = snprintf(buf, sizeof buf, "%d ", (int)sex[i]); out.append(buf, (size_t)n); }
        for (int c = 0; c < ncol; c++) { const int n = snprintf(buf, sizeof buf, "%g", cols[c][i]); out.append(buf, (size_t)n); out.push_back(c + 1 == ncol ? '\n' : ' '); }
    }
}

// ids [n][7], sex [n], cols: ncol pointers to n doubles each (per phenotype A D G C E F P, then MV SV SV_f).  -> 0, *bytes = size of
// the rows; they are copied to out when cap suffices (-1 otherwise)
extern "C" int info_format_host(const int64_t* ids, const uint8_t* sex, const double* const* cols, int ncol, size_t n, int max_threads, char* out, size_t cap, size_t* bytes)
{
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nt = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(hw ? hw : 1, (size_t)std::max(1, std::min(max_threads, 8))), n / 4096 + 1));
    std::vector<std::string> part(nt);
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; t++) th.emplace_back([&, t]() { format_rows(ids, sex, cols, ncol, n * t / nt, n * (t + 1) / nt, part[t]); });
    format_rows(ids, sex, cols, ncol, 0, n / nt, part[0]);
    for (auto& x : th) x.join();
    size_t total = 0;
    for (const std::string& p : part) total += p.size();
    *bytes = total;
    if (total > cap) return -1;
    size_t at = 0;
    for (const std::string& p : part) { memcpy(out + at, p.data(), p.size()); at += p.size(); }
    return 0;
}
