// gev_fmt_int.h -- one line of the .int interval file (Simulation::ras_write_hap_to_interval_format, src/Simulation.cpp:1582-1639), on
// the host and on the device from the same source.  Used by gev_format_interval_text (k_int_rows) and its host build
// (gev_dbg_format_interval_text_host).
//
//     <ID+1> <chr_label> <ihap> <st> <en> <hap_index+1> <name>.<1|2> <root_population+1>\n
//
// every number a plain decimal, name = the founder's .indv id, .1 for an even hap_index and .2 for an odd one (:3031-3033).
//
// Decimals.  A u64 is cut into pieces below 10^8 by multiply-high (v / 10^8 = mulhi(v, ceil(2^90 / 10^8)) >> 26, exact for every u64:
// tools/int_fmt_check.cpp), a piece into four digit pairs and a pair into two digits by 32-bit constant divisions, which compile to
// one multiply and a shift each: no divide instruction per digit.  The digit count comes from comparisons with the powers of ten.
// Digits go straight to the sink (the line's bytes in memory) at fixed distances from the number's end, each behind a test against
// the count: no per-thread array is indexed at run time, so a kernel that formats keeps nothing in scratch memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GEV_INT_HD __host__ __device__
#else
#define GEV_INT_HD
#endif

#define GEV_INT_NAME_MAX 64                 // bytes of a founder name (gev_set_founder_names refuses longer ones)
// the longest line: ID+1 (20) chr_label (11, with a sign) ihap (1) st (20) en (20) hap_index+1 (20) name.N (66) root_population+1 (11),
// seven spaces and the newline
#define GEV_INT_LINE_MAX (20 + 1 + 11 + 1 + 1 + 1 + 20 + 1 + 20 + 1 + 20 + 1 + (GEV_INT_NAME_MAX + 2) + 1 + 11 + 1)
#define GEV_INT_HEADER "h_ID chr hap st en hap_index gen0_indv root_pop\n"

GEV_INT_HD inline uint64_t gev_int_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
GEV_INT_HD inline uint64_t gev_int_div1e8(uint64_t v) { return gev_int_mulhi(v, 0xABCC77118461CEFDull) >> 26; }

// decimal digits of v
GEV_INT_HD inline uint32_t gev_int_dec_len(uint64_t v)
{
    if (!(v >> 32)) {
        const uint32_t w = (uint32_t)v;
        return 1u + (w >= 10u) + (w >= 100u) + (w >= 1000u) + (w >= 10000u) + (w >= 100000u) + (w >= 1000000u) + (w >= 10000000u) + (w >= 100000000u) + (w >= 1000000000u);
    }
    return 10u + (v >= 10000000000ull) + (v >= 100000000000ull) + (v >= 1000000000000ull) + (v >= 10000000000000ull) + (v >= 100000000000000ull) + (v >= 1000000000000000ull)
               + (v >= 10000000000000000ull) + (v >= 100000000000000000ull) + (v >= 1000000000000000000ull) + (v >= 10000000000000000000ull);
}
// the low min(n, 8) digits of w < 10^8, the last of them at end - 1.  Sink: put(position, byte)
template <class Sink>
GEV_INT_HD inline void gev_int_put8(Sink& s, uint32_t end, uint32_t w, uint32_t n)
{
    const uint32_t a = w / 10000u, b = w - a * 10000u;
    const uint32_t p3 = a / 100u, p2 = a - p3 * 100u, p1 = b / 100u, p0 = b - p1 * 100u;
    uint32_t t;
    t = p0 / 10u;              s.put(end - 1u, '0' + (p0 - t * 10u)); if (n > 1u) s.put(end - 2u, '0' + t);
    t = p1 / 10u; if (n > 2u)  s.put(end - 3u, '0' + (p1 - t * 10u)); if (n > 3u) s.put(end - 4u, '0' + t);
    t = p2 / 10u; if (n > 4u)  s.put(end - 5u, '0' + (p2 - t * 10u)); if (n > 5u) s.put(end - 6u, '0' + t);
    t = p3 / 10u; if (n > 6u)  s.put(end - 7u, '0' + (p3 - t * 10u)); if (n > 7u) s.put(end - 8u, '0' + t);
}
// v as a decimal at [pos, pos + n), n = gev_int_dec_len(v); returns pos + n
template <class Sink>
GEV_INT_HD inline uint32_t gev_int_dec(Sink& s, uint32_t pos, uint64_t v)
{
    const uint32_t n = gev_int_dec_len(v), end = pos + n;
    if (!(v >> 32)) {
        const uint32_t w = (uint32_t)v, hi = w / 100000000u;
        gev_int_put8(s, end, w - hi * 100000000u, n);
        if (n > 8u) gev_int_put8(s, end - 8u, hi, n - 8u);
    } else {                                                   // n >= 10
        const uint64_t r = gev_int_div1e8(v), top = gev_int_div1e8(r);
        gev_int_put8(s, end, (uint32_t)(v - r * 100000000ull), 8u);
        gev_int_put8(s, end - 8u, (uint32_t)(r - top * 100000000ull), n - 8u);
        if (n > 16u) gev_int_put8(s, end - 16u, (uint32_t)top, n - 16u);
    }
    return end;
}
GEV_INT_HD inline uint32_t gev_int_sdec_len(int v) { return v < 0 ? 1u + gev_int_dec_len((uint64_t)(-(int64_t)v)) : gev_int_dec_len((uint64_t)v); }
template <class Sink>
GEV_INT_HD inline uint32_t gev_int_sdec(Sink& s, uint32_t pos, int v)
{
    if (v < 0) { s.put(pos, '-'); return gev_int_dec(s, pos + 1u, (uint64_t)(-(int64_t)v)); }
    return gev_int_dec(s, pos, (uint64_t)v);
}

// the numbers of one line: id1 = (u64)(Human::ID + 1), hap1 = hap_index + 1, root1 = root_population + 1 (all as the reference's
// unsigned arithmetic gives them), ihap = 0 | 1
struct GevIntLine { uint64_t id1, st, en, hap1; uint32_t root1, ihap; int chr_label; };

// bytes of the line, its founder name name_len bytes long
GEV_INT_HD inline uint32_t gev_int_line_len(const GevIntLine& l, uint32_t name_len)
{
    return gev_int_dec_len(l.id1) + gev_int_sdec_len(l.chr_label) + gev_int_dec_len(l.st) + gev_int_dec_len(l.en) + gev_int_dec_len(l.hap1) + name_len + gev_int_dec_len(l.root1) + 11u;
}
// the line at [pos, ...) of the sink; returns the position behind its newline (= pos + gev_int_line_len)
template <class Sink>
GEV_INT_HD inline uint32_t gev_int_line(Sink& s, uint32_t pos, const GevIntLine& l, const unsigned char* __restrict__ name, uint32_t name_len)
{
    pos = gev_int_dec(s, pos, l.id1); s.put(pos++, ' ');
    pos = gev_int_sdec(s, pos, l.chr_label); s.put(pos++, ' ');
    s.put(pos++, '0' + l.ihap); s.put(pos++, ' ');
    pos = gev_int_dec(s, pos, l.st); s.put(pos++, ' ');
    pos = gev_int_dec(s, pos, l.en); s.put(pos++, ' ');
    pos = gev_int_dec(s, pos, l.hap1); s.put(pos++, ' ');
    for (uint32_t k = 0; k < name_len; k++) s.put(pos++, name[k]);
    s.put(pos++, '.'); s.put(pos++, (l.hap1 & 1u) ? '1' : '2'); s.put(pos++, ' ');        // hap_index even: hap1 odd
    pos = gev_int_dec(s, pos, l.root1); s.put(pos++, '\n');
    return pos;
}
// sink of the host build: plain memory
struct GevIntMemSink { char* p; GEV_INT_HD void put(uint32_t pos, uint32_t c) { p[pos] = (char)c; } };
