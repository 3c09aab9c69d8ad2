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
// 64-bit operand word for both kinds, against 6 matrix steps.  The order inside a step is free as long as both operands share it: a
// permutation of the summation index cancels in the sum.
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
#include <vector>
#include "gev_paircount.h"                         // gev_pc_range_mask, gev_pc_popcount64

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
// words of a SNP-major row that hold a haplotype of [hap_begin, +n_hap), padded to the 4 words one product step takes
inline size_t gev_ld_words4(size_t hap_begin, size_t n_hap) { return n_hap ? (((hap_begin + n_hap - 1) >> 6) - (hap_begin >> 6) + 1 + 3) & ~(size_t)3 : 0; }

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
        n_w4 = gev_ld_words4(h0, nh);
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
                        for (int st = 0; st < 2; st++) {
                            gev_ld_expand_hap(w32, st, e);
                            for (int q = 0; q < 4; q++) for (int b = 0; b < 4; b++) hb[(s * n_w4 + w) * 64 + 32 * half + 16 * st + 4 * q + b] = (int8_t)(e[q] >> (8 * b));
                        }
                    if (want_gen) {
                        gev_ld_expand_gen(w32, e);
                        for (int q = 0; q < 4; q++) for (int b = 0; b < 4; b++) gb[(s * n_w4 + w) * 32 + 16 * half + 4 * q + b] = (int8_t)(e[q] >> (8 * b));
                    }
                }
            }
        }
    }
    // the accumulator of the matrix instruction for SNP i of this side and SNP k of o
    uint32_t product(bool genotype, size_t i, const gev_ld_side_host& o, size_t k) const
    {
        const size_t nb = n_w4 * (genotype ? 32 : 64);
        const int8_t* a = (genotype ? gb.data() : hb.data()) + i * nb; const int8_t* b = (genotype ? o.gb.data() : o.hb.data()) + k * nb;
        int32_t acc = 0;
        for (size_t j = 0; j < nb; j++) acc += (int32_t)a[j] * b[j];
        return (uint32_t)acc;
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
// The device.  Both kernels work on SNP-major rows (snp_major_device: transposed from the resident planes, mutation overlay applied).
//
// 1. k_ld_prep: one wave per SNP walks the words of the haplotype range (lane = word, coalesced), writes the masked words into the
// side's plane and reduces c, n_het, n_hom_alt over the wave.  The plane is WORD-major: plane[w * n_pad + snp], so that the product's
// 16 lanes of a fragment row read 16 consecutive words.  It is padded to LD_TILE SNPs and to 4 words with zeros (a zero operand adds
// nothing to any sum), so the product needs no bounds on its loads.  One plane serves both products.
//
// 2. k_ld_product: v_mfma_i32_16x16x64_i8, exact i32 accumulators.  A workgroup of four waves owns a tile of SNP pairs and the whole
// haplotype range: no split over the summation index.  A wave owns 16 FR x 16 FR pairs; per step of 256 haplotypes lane (r = lane &
// 15, q = lane >> 4) loads ONE word per fragment -- word 4 W + q of SNP r -- which feeds four haplotype or two genotype matrix steps.
// A row = lane & 15, B column = lane & 15, C/D column = lane & 15 and row = 4 (lane >> 4) + register; the order of the summation index
// inside a step is the same function of (lane, step) for both operands and cancels.  GEN: which of the two products is formed.
//   block form (SCORE false): the accumulators are stored, [n_a][n_b].
//   score form (SCORE true): per element the window test, the quantum from the accumulator and the per-SNP
//   counts, a sum along the tile's row over the fragments and the 16 lanes of a row, one 64-bit atomic add per row and wave.  A wave
//   whose pairs lie wholly outside the band leaves at once.  No pair matrix is written.
// Every store and atomic is a vector one.
// ------------------------------------------------------------------------------------------
#define LD_TILE 128u                              // SNPs the planes are padded to = the larger tile side
#define LD_SCORE_TILES_PER_CU 2u                  // score form: large tiles where the band touches at least this many of them per compute unit (measured)

// rows: SNP-major rows of n_snps SNPs (row_w64 words apart), which are SNPs [snp_off, +n_snps) of the side; the block writes SNPs
// [snp_off, +n_cover) of the plane, zeros beyond n_snps (the pad of the side).  plane: n_w4 words x n_pad SNPs; the three count vectors
// are indexed like the plane
__global__ void __launch_bounds__(256) k_ld_prep(const u64* __restrict__ rows, size_t row_w64, u32 n_snps, u32 n_cover, u32 snp_off, u32 n_pad,
                                                 u64 hap_begin, u64 n_hap, u32 n_w4, u64* __restrict__ plane,
                                                 u32* __restrict__ cnt_c, u32* __restrict__ cnt_het, u32* __restrict__ cnt_hom)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 s = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (s >= n_cover) return;
    const size_t w_first = (size_t)(hap_begin >> 6);
    const u32 n_w = n_hap ? (u32)(((hap_begin + n_hap - 1u) >> 6) - w_first + 1u) : 0u;
    u32 c = 0, het = 0, hom = 0;
    for (u32 w = lane; w < n_w4; w += 64u) {
        u64 v = 0;
        if (s < n_snps && w < n_w) {
            v = rows[(size_t)s * row_w64 + w_first + w] & gev_pc_range_mask(w_first + w, (size_t)hap_begin, (size_t)(hap_begin + n_hap));
            gev_ld_word_counts(v, c, het, hom);
        }
        plane[(size_t)w * n_pad + snp_off + s] = v;
    }
    if (s >= n_snps) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { c += __shfl_xor(c, d); het += __shfl_xor(het, d); hom += __shfl_xor(hom, d); }
    if (lane == 0) { cnt_c[snp_off + s] = c; cnt_het[snp_off + s] = het; cnt_hom[snp_off + s] = hom; }
}

// what the score form needs beside the planes
struct LdScoreArgs {
    const u32 *c_a, *het_a, *hom_a, *c_b, *het_b, *hom_b;     // the per-SNP counts of the two sides (indexed like the planes)
    const u32 *win_lo, *win_hi;                               // the windows of side A's SNPs (entry i = SNP i of the side)
    u64* score; u32* n_terms;                                 // what is added to (entry i = SNP i of side A); n_terms may be null
    u64 n_ind;
    u32 b_first;                                              // SNP index (within the chromosome) of side B's SNP 0
};

// planes of side A (n_pad_a SNPs) and side B (n_pad_b), n_w4 words each (a multiple of 4); block form: out row-major [n_a][n_b].  GEN: the
// genotype product (gg), otherwise the haplotype product (n11) -- one product per launch: a kernel that forms both holds 128 accumulators
// beside both operand sets, runs one wave per SIMD and was measured slower than the two launches.  FR: 16 x 16 fragments per
// wave and side (4: tiles of 128 x 128, 2: tiles of 64 x 64 for blocks too small to fill the device with the large ones).
// blockIdx.y = tile of A, blockIdx.x = tile of B
template <int FR, bool GEN, bool SCORE>
__global__ void __launch_bounds__(256) k_ld_product(const u64* __restrict__ pa_p, u32 n_pad_a, const u64* __restrict__ pb_p, u32 n_pad_b, u32 n_w4,
                                                    u32 n_a, u32 n_b, u32* __restrict__ out, LdScoreArgs sa)
{
    constexpr u32 WAVE = 16u * FR, TILE = 2u * WAVE;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u32 r = lane & 15u, q = lane >> 4;
    const u32 a0 = blockIdx.y * TILE + (wave >> 1) * WAVE, b0 = blockIdx.x * TILE + (wave & 1u) * WAVE;         // the wave's pairs
    if (a0 >= n_a || b0 >= n_b) return;                                                                        // (nothing of the wave's is stored)
    if (SCORE) {                                  // the windows are non-decreasing: the first row's begin and the last row's end bound the band
        const u32 i_last = (a0 + WAVE < n_a ? a0 + WAVE : n_a) - 1u;
        const u32 k_first = sa.b_first + b0, k_end = sa.b_first + (b0 + WAVE < n_b ? b0 + WAVE : n_b);
        if (k_end <= sa.win_lo[a0] || k_first >= sa.win_hi[i_last]) return;
    }
    pc_v4i acc[FR][FR];
#pragma unroll
    for (int m = 0; m < FR; m++)
#pragma unroll
        for (int n = 0; n < FR; n++) acc[m][n] = pc_v4i{0, 0, 0, 0};
    const u64* pa = pa_p + (size_t)q * n_pad_a + a0 + r;
    const u64* pb = pb_p + (size_t)q * n_pad_b + b0 + r;
    u64 wa[FR], wb[FR];                           // the step in hand
    u64 na[FR], nb[FR];                           // the next one, loaded while this one is multiplied
#pragma unroll
    for (int m = 0; m < FR; m++) { na[m] = pa[16 * m]; nb[m] = pb[16 * m]; }
    for (u32 W = 0; W < n_w4; W += 4u) {
#pragma unroll
        for (int m = 0; m < FR; m++) { wa[m] = na[m]; wb[m] = nb[m]; }
        if (W + 4u < n_w4) {
            pa += (size_t)4 * n_pad_a; pb += (size_t)4 * n_pad_b;
#pragma unroll
            for (int m = 0; m < FR; m++) { na[m] = pa[16 * m]; nb[m] = pb[16 * m]; }
        }
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
            for (int s = 0; s < (GEN ? 1 : 2); s++) {
                pc_v4i ea[FR], eb[FR];
#pragma unroll
                for (int m = 0; m < FR; m++) {
                    u32 e[4];
                    if (GEN) gev_ld_expand_gen((u32)(wa[m] >> (32 * half)), e); else gev_ld_expand_hap((u32)(wa[m] >> (32 * half)), s, e);
                    ea[m] = pc_v4i{(int)e[0], (int)e[1], (int)e[2], (int)e[3]};
                    if (GEN) gev_ld_expand_gen((u32)(wb[m] >> (32 * half)), e); else gev_ld_expand_hap((u32)(wb[m] >> (32 * half)), s, e);
                    eb[m] = pc_v4i{(int)e[0], (int)e[1], (int)e[2], (int)e[3]};
                }
#pragma unroll
                for (int m = 0; m < FR; m++)
#pragma unroll
                    for (int n = 0; n < FR; n++) acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ea[m], eb[n], acc[m][n], 0, 0, 0);
            }
    }
    // C/D: column = lane & 15, row = 4 (lane >> 4) + register
    if (!SCORE) {
#pragma unroll
        for (int n = 0; n < FR; n++) {
            const u32 k = b0 + 16u * n + r;
            if (k >= n_b) continue;
#pragma unroll
            for (int m = 0; m < FR; m++)
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const u32 i = a0 + 16u * m + 4u * q + v;
                    if (i >= n_a) continue;
                    out[(size_t)i * n_b + k] = (u32)acc[m][n][v];
                }
        }
    } else {
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
                    sum += gev_ld_r2_q40(gev_ld_num(GEN, sa.n_ind, (u32)acc[m][n][v], cj, ck[n]), den_j, den_k[n]);
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
