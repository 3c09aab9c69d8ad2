// int_format_host.cpp -- the host way to write a .int interval file, for tools/int_text_bench.py: C snprintf on up to 8 threads, each
// formatting a contiguous slice of the individuals, the slices copied out in order, on the lists gev_download_intervals returns.
// Build: g++ -O2 -std=c++14 -shared -fPIC -pthread tools/int_format_host.cpp -o tools/libint_format_host.so
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

struct Part { uint64_t st, en, hap_index; int32_t root_population, reserved; };      // = gev_part

static void format_rows(const Part* parts, const uint64_t* off, const int64_t* ids, int chr_label, const char* const* name_bytes, const uint32_t* const* name_offsets,
                        size_t i0, size_t i1, std::string& out)
{
    char buf[256];
    out.reserve((size_t)(off[2 * i1] - off[2 * i0]) * 48);
    for (size_t i = i0; i < i1; i++)
        for (int ihap = 0; ihap < 2; ihap++)
            for (uint64_t q = off[2 * i + ihap]; q < off[2 * i + ihap + 1]; q++) {
                const Part& p = parts[q];
                const uint32_t* no = name_offsets[p.root_population]; const uint64_t k = p.hap_index / 2;
                const int n = snprintf(buf, sizeof buf, "%lu %d %d %lu %lu %lu %.*s.%c %d\n", (unsigned long)(ids[i] + 1), chr_label, ihap, (unsigned long)p.st, (unsigned long)p.en,
                                       (unsigned long)(p.hap_index + 1), (int)(no[k + 1] - no[k]), name_bytes[p.root_population] + no[k], (p.hap_index & 1) ? '2' : '1', p.root_population + 1);
                out.append(buf, (size_t)n);
            }
}

// -> 0, *bytes = size of the lines (no header); they are copied to out when cap suffices (-1 otherwise)
extern "C" int int_format_host(const Part* parts, const uint64_t* off, const int64_t* ids, size_t n_ind, int chr_label, const char* const* name_bytes,
                               const uint32_t* const* name_offsets, int max_threads, char* out, size_t cap, size_t* bytes)
{
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nt = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(hw ? hw : 1, (size_t)std::max(1, std::min(max_threads, 8))), n_ind / 4096 + 1));
    std::vector<std::string> part(nt);
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; t++) th.emplace_back([&, t]() { format_rows(parts, off, ids, chr_label, name_bytes, name_offsets, n_ind * t / nt, n_ind * (t + 1) / nt, part[t]); });
    format_rows(parts, off, ids, chr_label, name_bytes, name_offsets, 0, n_ind / nt, part[0]);
    for (auto& x : th) x.join();
    size_t total = 0;
    for (const std::string& p : part) total += p.size();
    *bytes = total;
    if (total > cap) return -1;
    size_t at = 0;
    for (const std::string& p : part) { memcpy(out + at, p.data(), p.size()); at += p.size(); }
    return 0;
}
