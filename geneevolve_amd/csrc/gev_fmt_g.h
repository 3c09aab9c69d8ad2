// gev_fmt_g.h -- the bytes of printf("%g", v) (glibc; = the default ostream format of a double) for any double, on the host and on
// the device from the same source.  Used by the .info text writer (gev_format_info_text) and its host mirror (gev_dbg_format_g_host).
//
// %g with the default precision prints P = 6 significant digits of the EXACT binary value, rounded half to even, in exponential style
// when the decimal exponent X after rounding is < -4 or >= 6 and in fixed style otherwise, without trailing zeros or a bare point.
//
// Fast path.  v = m * 2^e2 with m in [2^52, 2^53) (subnormals are shifted up, e2 down to -1126).  For every e2 the table holds
//     xhi = floor(log10((2^53 - 1) * 2^e2))           the decimal exponent at the top of the binade (the bottom has xhi or xhi - 1)
//     t   = floor(2^e2 * 10^(6 - xhi) * 2^156)        < 2^128
// so q = m * 2^e2 * 10^(6 - xhi) lies in (5e5, 1e7): SEVEN digits at the top of the binade, six or seven below.  The 181-bit product
// m * t is q in fixed point with 156 fraction bits: I = its integer part, F = its top 64 fraction bits.  t is short of the true
// factor by less than 2^-156, the product therefore by less than m * 2^-156 < 2^-103, and the fraction bits below F are dropped:
//     F <= frac(q) * 2^64 < F + 2        (the integer part may be one short when F is within 2 of 2^64: see below)
// I < 10^6 : six digits, X = xhi - 1, D = I rounded on frac(q) against 1/2.  Decided unless F is within 2 of 2^63.
// I >= 10^6: seven digits, X = xhi, D = I / 10 rounded on (I % 10) + frac(q) against 5.  Decided unless I % 10 == 5 and F < 2, or
//            I % 10 == 4 and F >= 2^64 - 2.
// Rounding is monotone and D = 10^6 carries into X, so an integer part that is one short (true fraction just past 1) gives the same
// digits by either reading: only the neighbourhood of the rounding boundary itself is undecided.  There (and only there: a value
// that lies exactly on a boundary always lands in it) gev_fmt_g_exact repeats the decision in exact multi-word integers.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GEV_FMT_HD __host__ __device__
#else
#define GEV_FMT_HD
#endif
#define GEV_FMT_NOINLINE __attribute__((noinline))
// the exact path's word loops stay loops: unrolled, its four integers would be promoted to registers and every kernel that can reach
// the path would be given that register count
#if defined(__clang__)
#define GEV_FMT_LOOP _Pragma("clang loop unroll(disable)")
#else
#define GEV_FMT_LOOP
#endif

#define GEV_FMT_E2_MIN (-1126)
#define GEV_FMT_N 2098                      // e2 = -1126 .. 971
#define GEV_FMT_MAX 13                      // "-1.23456e-308"

struct GevFmtEnt { uint64_t lo, hi; };
struct GevFmtTables {
    GevFmtEnt t[GEV_FMT_N];
    int16_t xhi[GEV_FMT_N + 6];             // (padded: the struct is a multiple of 16 bytes)
};
static_assert(sizeof(GevFmtTables) % 16 == 0, "GevFmtTables must be a multiple of 16 bytes");

// the formatted bytes, first byte in the low bits of lo; NUL beyond len
struct GevG { uint64_t lo, hi; uint32_t len; };

GEV_FMT_HD inline void gev_g_put(GevG& o, uint32_t c)
{
    const uint32_t s = (o.len & 7u) * 8u;
    if (o.len < 8) o.lo |= (uint64_t)c << s; else o.hi |= (uint64_t)c << s;
    o.len++;
}
GEV_FMT_HD inline uint64_t gev_fmt_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// ---- exact path: little-endian integers of GEV_FMT_NW 32-bit words (the largest, m * 10^330 and 5 * 2^1126, have under 1160 bits)
#define GEV_FMT_NW 40
GEV_FMT_HD inline void gev_big_set(uint32_t* a, uint64_t v) { GEV_FMT_LOOP for (int i = 0; i < GEV_FMT_NW; i++) a[i] = 0; a[0] = (uint32_t)v; a[1] = (uint32_t)(v >> 32); }
GEV_FMT_HD inline void gev_big_copy(uint32_t* a, const uint32_t* b) { GEV_FMT_LOOP for (int i = 0; i < GEV_FMT_NW; i++) a[i] = b[i]; }
GEV_FMT_HD inline void gev_big_mul_small(uint32_t* a, uint32_t f)
{
    uint64_t carry = 0;
    GEV_FMT_LOOP for (int i = 0; i < GEV_FMT_NW; i++) { const uint64_t p = (uint64_t)a[i] * f + carry; a[i] = (uint32_t)p; carry = p >> 32; }
}
GEV_FMT_HD inline void gev_big_mul_pow10(uint32_t* a, int j)
{
    GEV_FMT_LOOP for (; j >= 9; j -= 9) gev_big_mul_small(a, 1000000000u);
    GEV_FMT_LOOP for (; j > 0; j--) gev_big_mul_small(a, 10u);
}
GEV_FMT_HD inline void gev_big_shl(uint32_t* a, int bits)
{
    const int w = bits >> 5, b = bits & 31;
    GEV_FMT_LOOP for (int i = GEV_FMT_NW - 1; i >= 0; i--) {
        const uint32_t hi = i - w >= 0 ? a[i - w] : 0u, lo = i - w - 1 >= 0 ? a[i - w - 1] : 0u;
        a[i] = b ? (hi << b) | (lo >> (32 - b)) : hi;
    }
}
GEV_FMT_HD inline int gev_big_cmp(const uint32_t* a, const uint32_t* b)
{
    GEV_FMT_LOOP for (int i = GEV_FMT_NW - 1; i >= 0; i--) if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
GEV_FMT_HD inline void gev_big_sub(uint32_t* a, const uint32_t* b)        // a -= b (a >= b)
{
    uint64_t borrow = 0;
    GEV_FMT_LOOP for (int i = 0; i < GEV_FMT_NW; i++) { const uint64_t d = (uint64_t)a[i] - b[i] - borrow; a[i] = (uint32_t)d; borrow = (d >> 32) & 1u; }
}
GEV_FMT_HD inline void gev_big_add(uint32_t* a, const uint32_t* b)
{
    uint64_t carry = 0;
    GEV_FMT_LOOP for (int i = 0; i < GEV_FMT_NW; i++) { const uint64_t s = (uint64_t)a[i] + b[i] + carry; a[i] = (uint32_t)s; carry = s >> 32; }
}
// q = m * 2^e2 * 10^(6 - xhi) = A / B in integers; I = the fast path's integer part of q (at most one off).  -> the six digits D
// (10^6 when the rounding carried) and their decimal exponent X, rounded half to even on the exact remainder.
GEV_FMT_HD GEV_FMT_NOINLINE inline void gev_fmt_g_exact(uint64_t m, int e2, int xhi, uint32_t I, uint32_t* D_out, int* X_out)
{
    uint32_t A[GEV_FMT_NW], B[GEV_FMT_NW], R[GEV_FMT_NW], W[GEV_FMT_NW];
    const int j = 6 - xhi;
    gev_big_set(A, m); gev_big_set(B, 1);
    if (e2 >= 0) gev_big_shl(A, e2); else gev_big_shl(B, -e2);
    if (j >= 0) gev_big_mul_pow10(A, j); else gev_big_mul_pow10(B, -j);
    gev_big_copy(W, B); gev_big_mul_small(W, I);                        // W = I * B
    while (gev_big_cmp(A, W) < 0) { I--; gev_big_sub(W, B); }
    gev_big_copy(R, A); gev_big_sub(R, W);
    while (gev_big_cmp(R, B) >= 0) { I++; gev_big_sub(R, B); }           // A = I * B + R, 0 <= R < B
    uint32_t D; int X, c;
    if (I < 1000000u) {
        X = xhi - 1; D = I;
        gev_big_shl(R, 1);
        c = gev_big_cmp(R, B);                                          // 2 R against B
    } else {
        X = xhi; D = I / 10u;
        gev_big_copy(W, B); gev_big_mul_small(W, I - D * 10u); gev_big_add(W, R);      // (I % 10) * B + R
        gev_big_copy(A, B); gev_big_mul_small(A, 5u);
        c = gev_big_cmp(W, A);                                          // against 5 B
    }
    if (c > 0 || (c == 0 && (D & 1u))) D++;
    *D_out = D; *X_out = X;
}

// -> the number of bytes (<= GEV_FMT_MAX); *exact = 1 when the exact path decided the rounding (else untouched).  FORCE_EXACT (the
// stand-alone checker): every finite value takes the exact path
template <bool FORCE_EXACT = false>
GEV_FMT_HD inline uint32_t gev_fmt_g(const GevFmtTables* __restrict__ T, double v, GevG& o, uint32_t* exact)
{
    uint64_t b; memcpy(&b, &v, 8);
    const uint32_t E = (uint32_t)(b >> 52) & 0x7ffu;
    uint64_t m = b & ((1ull << 52) - 1);
    o.lo = 0; o.hi = 0; o.len = 0;
    if (b >> 63) gev_g_put(o, '-');
    if (E == 0x7ffu) {
        if (m) { gev_g_put(o, 'n'); gev_g_put(o, 'a'); gev_g_put(o, 'n'); }
        else { gev_g_put(o, 'i'); gev_g_put(o, 'n'); gev_g_put(o, 'f'); }
        return o.len;
    }
    if (E == 0 && m == 0) { gev_g_put(o, '0'); return o.len; }
    int e2;
    if (E) { m |= 1ull << 52; e2 = (int)E - 1075; }
    else { const int s = __builtin_clzll(m) - 11; m <<= s; e2 = -1074 - s; }
    const GevFmtEnt ent = T->t[e2 - GEV_FMT_E2_MIN];
    const int xhi = T->xhi[e2 - GEV_FMT_E2_MIN];
    // m * (hi:lo) >> 156: words w2:w1:(w0) of the 192-bit product
    const uint64_t p0hi = gev_fmt_mulhi(m, ent.lo), p1lo = m * ent.hi, p1hi = gev_fmt_mulhi(m, ent.hi);
    const uint64_t w1 = p0hi + p1lo, w2 = p1hi + (w1 < p0hi ? 1u : 0u);
    const uint32_t I = (uint32_t)(w2 >> 28);
    const uint64_t F = (w2 << 36) | (w1 >> 28);
    uint32_t D; int X; bool near;
    if (I < 1000000u) {
        X = xhi - 1; D = I + (F > 0x8000000000000000ull ? 1u : 0u);
        near = F - 0x7ffffffffffffffcull < 8u;                          // (a little wider than the bound needs)
    } else {
        X = xhi; D = I / 10u;
        const uint32_t r = I - D * 10u;
        D += r >= 5u ? 1u : 0u;
        near = (r == 5u && F < 4u) || (r == 4u && F > 0xfffffffffffffffbull);
    }
    if (near || FORCE_EXACT) { gev_fmt_g_exact(m, e2, xhi, I, &D, &X); if (exact) *exact = 1; }
    if (D == 1000000u) { D = 100000u; X++; }
    // six digits in nibbles, digit i at bit 4 i (no array: a runtime index would put it in scratch memory)
    uint32_t dg = 0, q = D, nz = 0; bool tail = true;
#pragma unroll
    for (int i = 5; i >= 0; i--) { const uint32_t d = q % 10u; q /= 10u; dg |= d << (4 * i); if (tail && d == 0) nz++; else tail = false; }
    const int P = 6 - (int)nz;                                          // significant digits left (D >= 10^5: at least 1)
    if (X < -4 || X >= 6) {
        gev_g_put(o, '0' + (dg & 15u));
        if (P > 1) {
            gev_g_put(o, '.');
#pragma unroll
            for (int i = 1; i < 6; i++) if (i < P) gev_g_put(o, '0' + ((dg >> (4 * i)) & 15u));
        }
        gev_g_put(o, 'e'); gev_g_put(o, X < 0 ? '-' : '+');
        uint32_t a = (uint32_t)(X < 0 ? -X : X);
        if (a >= 100u) { gev_g_put(o, '0' + a / 100u); a %= 100u; }
        gev_g_put(o, '0' + a / 10u); gev_g_put(o, '0' + a % 10u);
    } else if (X >= 0) {
        const int nd = P > X + 1 ? P : X + 1;
#pragma unroll
        for (int i = 0; i < 6; i++) if (i < nd) { if (i == X + 1) gev_g_put(o, '.'); gev_g_put(o, '0' + ((dg >> (4 * i)) & 15u)); }
    } else {
        gev_g_put(o, '0'); gev_g_put(o, '.');
#pragma unroll
        for (int k = 0; k < 3; k++) if (k < -X - 1) gev_g_put(o, '0');
#pragma unroll
        for (int i = 0; i < 6; i++) if (i < P) gev_g_put(o, '0' + ((dg >> (4 * i)) & 15u));
    }
    return o.len;
}

// ---- host: the table (built once per process, as GevRngTables is) -------------------------------------------------------------------
#include <vector>
namespace gev_fmt_host {
typedef std::vector<uint32_t> Big;      // little endian
inline void mul_small(Big& a, uint32_t f) { uint64_t c = 0; for (auto& w : a) { const uint64_t p = (uint64_t)w * f + c; w = (uint32_t)p; c = p >> 32; } if (c) a.push_back((uint32_t)c); }
inline void div_small(Big& a, uint32_t d) { uint64_t r = 0; for (size_t i = a.size(); i-- > 0;) { const uint64_t x = (r << 32) | a[i]; a[i] = (uint32_t)(x / d); r = x % d; } }
inline Big pow2(int k) { Big a((size_t)k / 32 + 1, 0u); a[(size_t)k / 32] = 1u << (k % 32); return a; }
inline void shr(Big& a, int bits)
{
    const size_t w = (size_t)bits / 32; const int b = bits % 32;
    Big r(a.size(), 0u);
    for (size_t i = 0; i + w < a.size(); i++) { const uint32_t lo = a[i + w], hi = i + w + 1 < a.size() ? a[i + w + 1] : 0u; r[i] = b ? (lo >> b) | (hi << (32 - b)) : lo; }
    a.swap(r);
}
inline uint32_t word(const Big& a, size_t i) { return i < a.size() ? a[i] : 0u; }
// floor(2^e2 * 10^(6 - x) * 2^156); false when it does not fit 128 bits
inline bool entry(int e2, int x, GevFmtEnt& out)
{
    const int j = 6 - x, sh = e2 + 156;
    Big a;
    if (j >= 0) {
        a = Big(1, 1u);
        for (int k = 0; k < j; k++) mul_small(a, 10u);
        if (sh >= 0) { Big p = pow2(sh); Big r(a.size() + p.size() + 1, 0u); const size_t w = (size_t)sh / 32; const int b = sh % 32;
                       for (size_t i = 0; i < a.size(); i++) { const uint64_t x2 = (uint64_t)a[i] << b; r[i + w] |= (uint32_t)x2; r[i + w + 1] |= (uint32_t)(x2 >> 32); } a.swap(r); }
        else shr(a, -sh);
    } else {
        if (sh < 0) return false;
        a = pow2(sh);
        for (int k = 0; k < -j; k++) div_small(a, 10u);      // nested floors of an integer = the floor of the whole quotient
    }
    for (size_t i = 4; i < a.size(); i++) if (a[i]) return false;
    out.lo = (uint64_t)word(a, 0) | ((uint64_t)word(a, 1) << 32);
    out.hi = (uint64_t)word(a, 2) | ((uint64_t)word(a, 3) << 32);
    return true;
}
// integer part of (2^53 - 1) * t / 2^156
inline uint64_t top_of_binade(const GevFmtEnt& t)
{
    const uint64_t m = (1ull << 53) - 1;
    const unsigned __int128 p0 = (unsigned __int128)m * t.lo, p1 = (unsigned __int128)m * t.hi + (p0 >> 64);
    return (uint64_t)(p1 >> (156 - 64));
}
}  // namespace gev_fmt_host
inline void gev_fmt_build_tables(GevFmtTables& T)
{
    memset(&T, 0, sizeof T);
    for (int e2 = GEV_FMT_E2_MIN; e2 < GEV_FMT_E2_MIN + GEV_FMT_N; e2++) {
        // floor((e2 + 53) * log10(2)) as a first guess, then moved until the top of the binade has seven digits
        int x = (int)(((long long)(e2 + 53) * 1292913986LL) >> 32);
        GevFmtEnt ent{0, 0};
        for (int tries = 0; tries < 4; tries++) {
            if (!gev_fmt_host::entry(e2, x, ent)) { x++; continue; }
            const uint64_t top = gev_fmt_host::top_of_binade(ent);
            if (top < 1000000u) x--; else if (top >= 10000000u) x++; else break;
        }
        T.t[e2 - GEV_FMT_E2_MIN] = ent; T.xhi[e2 - GEV_FMT_E2_MIN] = (int16_t)x;
    }
}
inline const GevFmtTables& gev_fmt_host_tables()
{
    static const GevFmtTables* T = [] { GevFmtTables* t = new GevFmtTables; gev_fmt_build_tables(*t); return t; }();
    return *T;
}
