// gev_ldcount.h -- linkage disequilibrium per PAIR of SNPs from the SNP-major bit rows (gev_ld_counts, gev_ld_scores): the counts that
// haplotype r^2, D', genotype r^2 and LD scores are made of.  The reference has no such output; the truth it is held to is numpy over
// the rows gev_download_haps returns.
//
// A SNP-major row is one SNP: bit h = haplotype row h, bits 2i and 2i+1 = individual i.  Over individuals [ind_begin, +n_ind) of one
// population the sums run over n = 2 n_ind haplotypes and N = n_ind individuals.  Every word of a row is cut to the haplotype range
// [2 ind_begin, 2 ind_begin + 2 n_ind) with gev_pc_range_mask, so that pad bits and haplotypes outside the range are 0 in every
// operand and drop out of every sum; the range begins and ends on an even bit, so an individual's two bits are never parted.
// Per SNP (gev_ld_word_counts)
//     c = |w|                       allele-1 count            (= sum g)
//     n_het = |(w ^ w>>1) & 0x55..|   n_hom_alt = |(w & w>>1) & 0x55..|     (sum g^2 = n_het + 4 n_hom_alt)
// and per pair of SNPs two integer products
//     n11 = sum_h a_h b_h   (0/1 bytes, one per haplotype)          gg = sum_i g_i g'_i   (0/1/2 bytes, one per individual)
//
// The products run on bytes.  Bits become bytes in registers, per 32-bit half word of the ONE plane a side has:
//     haplotype bytes   e[j] = (w >> j) & 0x01010101, j = 0..7       byte b of e[j] = haplotype 8 b + j: 32 bytes, two matrix steps
//     genotype bytes    v = w - ((w >> 1) & 0x55555555)               every bit pair becomes its popcount
//                       g[j] = (v >> 2 j) & 0x03030303, j = 0..3     byte b of g[j] = individual 4 b + j: 16 bytes, one matrix step
// 16 operations for the 32 haplotype bytes (j = 0 needs no shift: 15), 3 + 7 for the 16 genotype bytes: 25 per half word, 50 per
// 64-bit operand word for both kinds, against 6 matrix steps (the order inside a step is free: gev_bitprod.h).
//
// r^2 is formed in integers as far as it goes and then in four separately rounded IEEE double operations (gev_ld_r2_q40): the
// quantum llrint(r^2 * 2^40).  An LD score is an integer sum of quanta, so the order of the sum is free.
//
// The first part of this file is plain C++ (host and device from one source: gev_dbg_ld_host runs the same masking, expansion,
// finishing and quantum code with a plain integer loop in place of the matrix instruction, and so does any host program that
// includes this file alone); the kernels behind it need gev_kernels.h (u32, u64).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>
#include <vector>
#include "gev_bitprod.h"                           // GEV_PC_HD, gev_pc_range_mask, gev_pc_popcount64, the product and the preparation walk

#define GEV_LD_MAX_IND ((size_t)1 << 30)          // gg can reach 4 n_ind, n11 2 n_ind
#define GEV_LD_Q40 1099511627776.0                // 2^40

// the counts of one (masked) word of a SNP's row, added to c / n_het / n_hom_alt
GEV_PC_HD inline void gev_ld_word_counts(uint64_t w, uint32_t& c, uint32_t& n_het, uint32_t& n_hom_alt)
{
    const uint64_t a = w & 0x5555555555555555ull, b = (w >> 1) & 0x5555555555555555ull;
    c += gev_pc_popcount64(w); n_het += gev_pc_popcount64(a ^ b); n_hom_alt += gev_pc_popcount64(a & b);
}
// haplotype bytes of a 32-bit half word: step s (0, 1) takes shifts 4 s .. 4 s + 3
GEV_PC_HD inline void gev_ld_expand_hap(uint32_t w, int s, uint32_t e[4])
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) e[j] = (w >> (4 * s + j)) & 0x01010101u;
}
// genotype bytes of a 32-bit half word (16 individuals)
GEV_PC_HD inline void gev_ld_expand_gen(uint32_t w, uint32_t g[4])
{
    const uint32_t v = w - ((w >> 1) & 0x55555555u);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) g[j] = (v >> (2 * j)) & 0x03030303u;
}
// denominator of a SNP: haplotype r^2  c (n - c);  genotype r^2  N sum g^2 - s^2  (both < 2^63 for n_ind <= 2^30)
GEV_PC_HD inline uint64_t gev_ld_den(bool genotype, uint64_t n_ind, uint32_t c, uint32_t n_het, uint32_t n_hom_alt)
{
    return genotype ? n_ind * ((uint64_t)n_het + 4ull * n_hom_alt) - (uint64_t)c * c : (uint64_t)c * (2 * n_ind - c);
}
// numerator of a pair: haplotype  n n11 - c_j c_k;  genotype  N gg - s_j s_k
GEV_PC_HD inline int64_t gev_ld_num(bool genotype, uint64_t n_ind, uint32_t product, uint32_t c_j, uint32_t c_k)
{
    return (int64_t)((genotype ? n_ind : 2 * n_ind) * (uint64_t)product) - (int64_t)((uint64_t)c_j * c_k);
}
// llrint(num^2 / (den_j den_k) * 2^40), 0 where a SNP is monomorphic.  Three conversions, two products, one quotient and one exact
// scaling, each rounded to nearest even on its own; there is no addition among them, so nothing can be contracted to an FMA.
GEV_PC_HD inline uint64_t gev_ld_r2_q40(int64_t num, uint64_t den_j, uint64_t den_k)
{
    if (den_j == 0 || den_k == 0) return 0;
    const double x = (double)num;
    const double nn = x * x, dd = (double)den_j * (double)den_k;
    const double r2 = nn / dd;                     // (the device's f64 quotient is the correctly rounded one unless fast-math is asked for)
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double2ll_rn(r2 * GEV_LD_Q40);
#else
    return (uint64_t)llrint(r2 * GEV_LD_Q40);
#endif
}
// One side on the host: SNPs [s0, +ns) of haplotype-major rows (row r = bits + r * stride words, SNP j = bit j & 63 of word j >> 6)
// turned SNP-major over haplotypes [2 ind_begin, +2 n_ind), masked, counted and expanded to the operand bytes of the device's order.
// Only the rows of the range and, of each, the words that hold a SNP of the side are read.
struct gev_ld_side_host {
    size_t ns = 0, n_w4 = 0;
    std::vector<uint32_t> c, het, hom;
    std::vector<int8_t> hb, gb;                    // [ns][n_w4 * 64], [ns][n_w4 * 32]
    gev_ld_side_host(const uint64_t* bits, size_t stride, size_t s0, size_t n_snps, size_t ind_begin, size_t n_ind, bool want_hap, bool want_gen)
    {
        ns = n_snps;
        const size_t h0 = 2 * ind_begin, nh = 2 * n_ind, w_first = h0 >> 6;
        n_w4 = gev_bp_words4(h0, nh);
        c.assign(ns, 0); het.assign(ns, 0); hom.assign(ns, 0);
        if (want_hap) hb.assign(ns * n_w4 * 64, 0);
        if (want_gen) gb.assign(ns * n_w4 * 32, 0);
        std::vector<uint64_t> row(n_w4);
        for (size_t s = 0; s < ns; s++) {
            const size_t j = s0 + s;
            for (size_t w = 0; w < n_w4; w++) row[w] = 0;
            for (size_t h = h0; h < h0 + nh; h++) row[(h >> 6) - w_first] |= ((bits[h * stride + (j >> 6)] >> (j & 63)) & 1ull) << (h & 63);
            for (size_t w = 0; w < n_w4; w++) {
                const uint64_t v = row[w] & gev_pc_range_mask(w_first + w, h0, h0 + nh);
                gev_ld_word_counts(v, c[s], het[s], hom[s]);
                for (int half = 0; half < 2; half++) {
                    const uint32_t w32 = (uint32_t)(v >> (32 * half));
                    uint32_t e[4];
                    if (want_hap)
                        for (int st = 0; st < 2; st++) { gev_ld_expand_hap(w32, st, e); gev_bp_store16(e, &hb[(s * n_w4 + w) * 64 + 32 * half + 16 * st]); }
                    if (want_gen) { gev_ld_expand_gen(w32, e); gev_bp_store16(e, &gb[(s * n_w4 + w) * 32 + 16 * half]); }
                }
            }
        }
    }
    // the accumulator of the matrix instruction for SNP i of this side and SNP k of o
    uint32_t product(bool genotype, size_t i, const gev_ld_side_host& o, size_t k) const
    {
        const size_t nb = n_w4 * (genotype ? 32 : 64);
        const std::vector<int8_t> &a = genotype ? gb : hb, &b = genotype ? o.gb : o.hb;
        return gev_bp_dot_i8(a.data() + i * nb, b.data() + k * nb, nb);
    }
    void copy_counts(uint32_t* oc, uint32_t* ohet, uint32_t* ohom) const
    {
        for (size_t s = 0; s < ns; s++) { if (oc) oc[s] = c[s]; if (ohet) ohet[s] = het[s]; if (ohom) ohom[s] = hom[s]; }
    }
};
// the block form: SNPs [a_begin, +n_a) of rows_a against SNPs [b_begin, +n_b) of rows_b (the same rows, or another chromosome's of the
// same population), matrices row-major [n_a][n_b]; each output may be NULL
inline void gev_ld_counts_host(const uint64_t* bits_a, size_t stride_a, size_t a_begin, size_t n_a, const uint64_t* bits_b, size_t stride_b, size_t b_begin, size_t n_b,
                               size_t ind_begin, size_t n_ind, uint32_t* n11, uint32_t* gg,
                               uint32_t* c_a, uint32_t* het_a, uint32_t* hom_a, uint32_t* c_b, uint32_t* het_b, uint32_t* hom_b)
{
    const gev_ld_side_host A(bits_a, stride_a, a_begin, n_a, ind_begin, n_ind, n11 != nullptr, gg != nullptr);
    const gev_ld_side_host B(bits_b, stride_b, b_begin, n_b, ind_begin, n_ind, n11 != nullptr, gg != nullptr);
    A.copy_counts(c_a, het_a, hom_a); B.copy_counts(c_b, het_b, hom_b);
    for (size_t i = 0; i < n_a; i++)
        for (size_t k = 0; k < n_b; k++) {
            if (n11) n11[i * n_b + k] = A.product(false, i, B, k);
            if (gg) gg[i * n_b + k] = A.product(true, i, B, k);
        }
}
// the score form: for SNP snp_begin + t the quanta of the SNPs [win_lo[t], win_hi[t]) of the same rows summed (windows already
// checked: non-decreasing, win_lo[t] <= snp_begin + t < win_hi[t] <= L); each output may be NULL
inline void gev_ld_scores_host(const uint64_t* bits, size_t stride, size_t snp_begin, size_t n_snps, const uint32_t* win_lo, const uint32_t* win_hi,
                               size_t ind_begin, size_t n_ind, bool genotype, uint64_t* score_q40, uint32_t* n_terms)
{
    if (!n_snps) return;
    const size_t u0 = win_lo[0], u1 = win_hi[n_snps - 1];
    const gev_ld_side_host A(bits, stride, snp_begin, n_snps, ind_begin, n_ind, !genotype, genotype);
    const gev_ld_side_host B(bits, stride, u0, u1 - u0, ind_begin, n_ind, !genotype, genotype);
    for (size_t t = 0; t < n_snps; t++) {
        const uint64_t den_j = gev_ld_den(genotype, n_ind, A.c[t], A.het[t], A.hom[t]);
        uint64_t sum = 0; uint32_t terms = 0;
        for (size_t k = win_lo[t]; k < win_hi[t]; k++) {
            const size_t b = k - u0;
            const uint64_t den_k = gev_ld_den(genotype, n_ind, B.c[b], B.het[b], B.hom[b]);
            terms += den_k != 0;
            sum += gev_ld_r2_q40(gev_ld_num(genotype, n_ind, A.product(genotype, t, B, b), A.c[t], B.c[b]), den_j, den_k);
        }
        if (score_q40) score_q40[t] = sum;
        if (n_terms) n_terms[t] = terms;
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// The device (the walk and the product: gev_bitprod.h).  Both kernels work on SNP-major rows (snp_major_device: transposed from the
// resident planes, mutation overlay applied).
//
// k_ld_prep: a row of the side is a SNP; its masked words go into the side's one plane, which serves both products.
// k_ld_product: one plane a side, one accumulator set; a word feeds four haplotype or two genotype matrix steps (GEN: which).
//   block form (SCORE false): the accumulators are stored, [n_a][n_b].
//   score form (SCORE true): per element the window test, the quantum from the accumulator and the per-SNP
//   counts, a sum along the tile's row over the fragments and the 16 lanes of a row, one 64-bit atomic add per row and wave.  A wave
//   whose pairs lie wholly outside the band leaves at once.  No pair matrix is written.
// Every store and atomic is a vector one.
// ------------------------------------------------------------------------------------------
#define LD_SCORE_TILES_PER_CU 2u                  // score form: large tiles where the band touches at least this many of them per compute unit (measured)

struct LdRow {
    static constexpr int NPLANES = 1;
    typedef BpSums<3, false> Sums;                // c, n_het, n_hom_alt
    const u64* rows; size_t row_w64;
    __device__ void word(u32 s, size_t w, u64 mask, u64 (&v)[1], Sums& sums) const { v[0] = rows[(size_t)s * row_w64 + w] & mask; gev_ld_word_counts(v[0], sums.s[0], sums.s[1], sums.s[2]); }
};
// rows: SNP-major rows of n_snps SNPs (row_w64 words apart), which are SNPs [snp_off, +n_snps) of the side; the block writes SNPs
// [snp_off, +n_cover) of the plane, zeros beyond n_snps (the pad of the side).  plane: n_w4 words x n_pad SNPs; the three count vectors
// are indexed like the plane
__global__ void __launch_bounds__(256) k_ld_prep(const u64* __restrict__ rows, size_t row_w64, u32 n_snps, u32 n_cover, u32 snp_off, u32 n_pad,
                                                 u64 hap_begin, u64 n_hap, u32 n_w4, u64* __restrict__ plane,
                                                 u32* __restrict__ cnt_c, u32* __restrict__ cnt_het, u32* __restrict__ cnt_hom)
{
    bp_prep(LdRow{rows, row_w64}, LdRow::Sums{{0, 0, 0}, 0, {cnt_c, cnt_het, cnt_hom}, nullptr}, n_snps, n_cover, snp_off, n_pad, hap_begin, n_hap, n_w4, {plane});
}

// what the score form needs beside the planes
struct LdScoreArgs {
    const u32 *c_a, *het_a, *hom_a, *c_b, *het_b, *hom_b;     // the per-SNP counts of the two sides (indexed like the planes)
    const u32 *win_lo, *win_hi;                               // the windows of side A's SNPs (entry i = SNP i of the side)
    u64* score; u32* n_terms;                                 // what is added to (entry i = SNP i of side A); n_terms may be null
    u64 n_ind;
    u32 b_first;                                              // SNP index (within the chromosome) of side B's SNP 0
};

struct LdHapProduct {                             // n11: 0/1 bytes, one per haplotype
    static constexpr int NPLANES = 1, NACC = 1, STEPS = 4;
    __device__ static void expand(const u64 (&w)[1], int s, pc_v4i (&f)[1]) { u32 e[4]; gev_ld_expand_hap((u32)(w[0] >> (32 * (s >> 1))), s & 1, e); f[0] = bp_v4(e); }
};
struct LdGenProduct {                             // gg: 0/1/2 bytes, one per individual
    static constexpr int NPLANES = 1, NACC = 1, STEPS = 2;
    __device__ static void expand(const u64 (&w)[1], int s, pc_v4i (&f)[1]) { u32 e[4]; gev_ld_expand_gen((u32)(w[0] >> (32 * s)), e); f[0] = bp_v4(e); }
};

// planes of side A (n_pad_a SNPs) and side B (n_pad_b), n_w4 words each; block form: out row-major [n_a][n_b].  GEN: the genotype
// product (gg), otherwise the haplotype product (n11) -- one product per launch: a kernel that forms both holds 128 accumulators
// beside both operand sets, runs one wave per SIMD and was measured slower than the two launches
template <int FR, bool GEN, bool SCORE>
__global__ void __launch_bounds__(256) k_ld_product(const u64* __restrict__ pa_p, u32 n_pad_a, const u64* __restrict__ pb_p, u32 n_pad_b, u32 n_w4,
                                                    u32 n_a, u32 n_b, u32* __restrict__ out, LdScoreArgs sa)
{
    using P = typename std::conditional<GEN, LdGenProduct, LdHapProduct>::type;
    constexpr u32 WAVE = 16u * FR;
    const u64* const pa[1] = {pa_p}; const u64* const pb[1] = {pb_p};
    const auto outside_band = [&](u32 a0, u32 b0) -> bool {   // the windows are non-decreasing: the first row's begin and the last row's end bound the band
        if (!SCORE) return false;
        const u32 i_last = (a0 + WAVE < n_a ? a0 + WAVE : n_a) - 1u;
        const u32 k_first = sa.b_first + b0, k_end = sa.b_first + (b0 + WAVE < n_b ? b0 + WAVE : n_b);
        return k_end <= sa.win_lo[a0] || k_first >= sa.win_hi[i_last];
    };
    u32 a0, b0; pc_v4i acc[1][FR][FR] = {};
    if (!bp_product<FR, P>(pa, n_pad_a, pb, n_pad_b, n_w4, n_a, n_b, outside_band, a0, b0, acc)) return;
    if (!SCORE) {
        bp_for_each<FR>(acc, a0, b0, n_a, n_b, [&](u32 i, u32 k, const u32 (&p)[1]) { out[(size_t)i * n_b + k] = p[0]; });
    } else {
        const u32 lane = threadIdx.x & 63u, r = lane & 15u, q = lane >> 4;
        u32 ck[FR], kk[FR]; u64 den_k[FR];        // the wave's columns of this lane: count, SNP index within the chromosome (none: ~0), denominator
#pragma unroll
        for (int n = 0; n < FR; n++) {
            const u32 k = b0 + 16u * n + r;
            const bool in = k < n_b;
            kk[n] = in ? sa.b_first + k : 0xFFFFFFFFu;
            ck[n] = in ? sa.c_b[k] : 0u;
            den_k[n] = in ? gev_ld_den(GEN, sa.n_ind, ck[n], sa.het_b[k], sa.hom_b[k]) : 0ull;
        }
#pragma unroll
        for (int m = 0; m < FR; m++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const u32 i = a0 + 16u * m + 4u * q + v;
                const bool row = i < n_a;
                const u32 lo = row ? sa.win_lo[i] : 0u, hi = row ? sa.win_hi[i] : 0u;          // (an empty window: nothing passes the test)
                const u32 cj = row ? sa.c_a[i] : 0u;
                const u64 den_j = row ? gev_ld_den(GEN, sa.n_ind, cj, sa.het_a[i], sa.hom_a[i]) : 0ull;
                u64 sum = 0; u32 terms = 0;
#pragma unroll
                for (int n = 0; n < FR; n++) {
                    if (kk[n] < lo || kk[n] >= hi) continue;
                    terms += den_k[n] != 0;
                    sum += gev_ld_r2_q40(gev_ld_num(GEN, sa.n_ind, (u32)acc[0][m][n][v], cj, ck[n]), den_j, den_k[n]);
                }
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1) { sum += __shfl_xor((unsigned long long)sum, d); terms += __shfl_xor(terms, d); }   // the 16 lanes of the row
                if (r == 0 && row) {
                    if (sum) atomicAdd((unsigned long long*)(sa.score + i), (unsigned long long)sum);
                    if (terms && sa.n_terms) atomicAdd(sa.n_terms + i, terms);
                }
            }
    }
}
#endif
