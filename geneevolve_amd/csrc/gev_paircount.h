// gev_paircount.h -- genotype counts per PAIR of individuals from the haplotype-major bit rows (gev_pair_genotype_counts,
// gev_ind_genotype_counts): what KING kinship, IBS distance and a VanRaden GRM are made of.  The reference has no such output; the
// truth it is held to is numpy over the rows gev_download_haps returns (g @ g.T, x @ x.T, y @ z.T + z @ y.T).
//
// Rows 2i and 2i+1 are individual i's haplotypes.  Per individual and 64-locus word
//     x = a ^ b   (heterozygous)        y = a & b   (allele 1 on both)
// both cut to the SNP range of the call (gev_pc_range_mask), so that pad bits and loci outside the range are 0 in both and drop out of
// every sum.  The genotype is g = x + 2y (0/1/2 copies of allele 1).  Two integer products per pair
//     xx = sum_j x_i x_k        gg = sum_j g_i g_k
// with the per-individual het = |x| and hom = |y| give the three outputs exactly (gev_pc_finish):
//     n_hethet = xx
//     dot      = gg
//     n_opphom = hom_i + hom_k - (gg - xx) / 2
// (gg - xx = 2 #{(1,2),(2,1)} + 4 #{(2,2)}, hom_i + hom_k = 2 #{(2,2)} + #{(1,2),(2,1)} + #{(2,0),(0,2)}: the difference is even and what
// is left are the loci where one is 0/0 and the other 1/1).  With h = g - 1 on the loci of the range (+1 / 0 / -1), hh = sum h_i h_k =
// gg - (2 hom_i + het_i) - (2 hom_k + het_k) + n_snps, so the same two products carry the signed form as well; g is the operand
// because its bytes cost less to make from bits (below), with no third plane and no range mask inside the product.
//
// The products run on bytes: one locus = one int8 of the operand.  Bits become bytes in registers, 16 loci (one matrix step of a lane)
// at a time, in the order in which masks alone find them (the order inside a step is free: gev_bitprod.h).  Of a 32-locus half word
// the loci of one parity are packed as 2-bit fields (gev_pc_pack2)
//     c = ((x >> parity) & 0x55555555) | (((y >> parity) & 0x55555555) << 1)          field f = g of locus 2 f + parity
// (x and y are disjoint, so the field is x + 2y), and four shifted masks turn c into the step's 16 bytes (gev_pc_expand)
//     g bytes[j] = (c >> 2j) & 0x03030303        byte b = g of field j + 4 b
//     x bytes[j] = g bytes[j] & 0x01010101       (g = 1 exactly where x)
// 14 operations per 16 loci for both operands.  A 64-locus word so feeds four steps: (low half, even), (low, odd), (high, even), (high, odd).
// The first part of this file is plain C++ (host and device from one source: gev_dbg_pair_counts_host runs the same masking, expansion
// and finishing code with a plain integer loop in place of the matrix instruction, and so does any host program that includes this
// file alone); the kernels behind it need gev_kernels.h (u32, u64).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "gev_bitprod.h"                           // GEV_PC_HD, gev_pc_range_mask, gev_pc_popcount64, the product and the preparation walk

#define GEV_PC_MAX_SNPS ((size_t)1 << 30)         // dot can reach 4 * n_snps

// one individual's word of the two planes from its two haplotype words
GEV_PC_HD inline void gev_pc_planes(uint64_t a, uint64_t b, uint64_t mask, uint64_t& x, uint64_t& y) { x = (a ^ b) & mask; y = (a & b) & mask; }
// the loci of one parity of a 32-locus half word as sixteen 2-bit fields: field f = g of locus 2 f + parity
GEV_PC_HD inline uint32_t gev_pc_pack2(uint32_t x32, uint32_t y32, unsigned parity)
{
    return ((x32 >> parity) & 0x55555555u) | (((y32 >> parity) & 0x55555555u) << 1);
}
// sixteen fields -> 16 bytes (four 32-bit words, field j + 4 b = byte b of word j): the g operand (0/1/2) and the x operand (0/1)
GEV_PC_HD inline void gev_pc_expand(uint32_t c, uint32_t g[4], uint32_t x[4])
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) { g[j] = (c >> (2 * j)) & 0x03030303u; x[j] = g[j] & 0x01010101u; }
}
// step s (0..3) of a 64-locus word of the two planes
GEV_PC_HD inline void gev_pc_expand_step(uint64_t xw, uint64_t yw, int s, uint32_t g[4], uint32_t x[4])
{
    gev_pc_expand(gev_pc_pack2((uint32_t)(xw >> (32 * (s >> 1))), (uint32_t)(yw >> (32 * (s >> 1))), (unsigned)(s & 1)), g, x);
}
// the three outputs of a pair from its two products and the per-individual counts
GEV_PC_HD inline void gev_pc_finish(uint32_t xx, uint32_t gg, uint32_t hom_i, uint32_t hom_k, uint32_t& n_hethet, uint32_t& n_opphom, uint32_t& dot)
{
    n_hethet = xx;
    dot = gg;
    n_opphom = hom_i + hom_k - ((gg - xx) >> 1);
}
// sum over the loci of a word of weight * g: weight[first + b] is the weight of the word's locus b (only loci with a bit in x | y are
// read, so first may be negative for a word the range begins in)
GEV_PC_HD inline uint64_t gev_pc_weighted(uint64_t x, uint64_t y, const uint32_t* weight, ptrdiff_t first)
{
    uint64_t sum = 0;
    for (uint64_t m = x | y; m; m &= m - 1) {
#if defined(__HIP_DEVICE_COMPILE__)
        const unsigned b = (unsigned)__ffsll((unsigned long long)m) - 1u;
#else
        const unsigned b = (unsigned)__builtin_ctzll(m);
#endif
        sum += (uint64_t)weight[first + (ptrdiff_t)b] << ((y >> b) & 1u);
    }
    return sum;
}

// Haplotype-major rows in host memory (row r = bits + r * row_stride_words, locus j = bit j & 63 of word j >> 6, rows 2i and 2i+1 =
// individual i).  Per individual of [0, n_ind): n_het / n_hom_alt over SNPs [snp_begin, +n_snps) (each may be NULL); per pair (i of
// [a_begin, +n_a), k of [b_begin, +n_b)), row-major [n_a][n_b], each may be NULL: the three counts.  Only the words that hold a SNP of
// the range are read.  The device's order of work: planes, operand bytes by the device's expansion, two integer products, finish.
inline void gev_pc_counts_host(const uint64_t* bits, size_t row_stride_words, size_t n_ind, size_t snp_begin, size_t n_snps,
                               size_t a_begin, size_t n_a, size_t b_begin, size_t n_b,
                               uint32_t* n_het, uint32_t* n_hom_alt, uint32_t* n_hethet, uint32_t* n_opphom, uint32_t* dot)
{
    const size_t snp_end = snp_begin + n_snps;
    const size_t w_first = snp_begin >> 6, n_w = n_snps ? ((snp_end - 1) >> 6) - w_first + 1 : 0;
    const size_t n_bytes = n_w * 64;
    std::vector<int8_t> xb(n_ind * n_bytes), gb(n_ind * n_bytes);
    std::vector<uint32_t> het(n_ind, 0), hom(n_ind, 0);
    for (size_t i = 0; i < n_ind; i++) {
        const uint64_t* ra = bits + 2 * i * row_stride_words; const uint64_t* rb = ra + row_stride_words;
        for (size_t w = 0; w < n_w; w++) {
            uint64_t x, y;
            gev_pc_planes(ra[w_first + w], rb[w_first + w], gev_pc_range_mask(w_first + w, snp_begin, snp_end), x, y);
            het[i] += gev_pc_popcount64(x); hom[i] += gev_pc_popcount64(y);
            for (int s = 0; s < 4; s++) {
                uint32_t xe[4], ge[4];
                gev_pc_expand_step(x, y, s, ge, xe);
                gev_bp_store16(xe, &xb[i * n_bytes + w * 64 + 16 * s]); gev_bp_store16(ge, &gb[i * n_bytes + w * 64 + 16 * s]);
            }
        }
        if (n_het) n_het[i] = het[i];
        if (n_hom_alt) n_hom_alt[i] = hom[i];
    }
    if (!n_hethet && !n_opphom && !dot) return;
    for (size_t i = 0; i < n_a; i++)
        for (size_t k = 0; k < n_b; k++) {
            const size_t ri = (a_begin + i) * n_bytes, rk = (b_begin + k) * n_bytes;
            const uint32_t xx = gev_bp_dot_i8(xb.data() + ri, xb.data() + rk, n_bytes), gg = gev_bp_dot_i8(gb.data() + ri, gb.data() + rk, n_bytes);
            uint32_t o_hethet, o_opphom, o_dot;
            gev_pc_finish(xx, gg, hom[a_begin + i], hom[b_begin + k], o_hethet, o_opphom, o_dot);
            if (n_hethet) n_hethet[i * n_b + k] = o_hethet;
            if (n_opphom) n_opphom[i * n_b + k] = o_opphom;
            if (dot) dot[i * n_b + k] = o_dot;
        }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// The device (the walk and the product: gev_bitprod.h).  Both kernels read STAGED rows (stage_rows_mutated: pool units resolved,
// mutation overlay applied, once per row).
//
// 1. k_pair_prep: a row of the side is an individual; its x and y words go into the two planes, n_het, n_hom_alt and, with weights,
// wsum are its counts.  gev_ind_genotype_counts is this kernel alone, without planes.
//
// 2. k_pair_product: two planes a side, two accumulator sets (xx, gg), four matrix steps per word (gev_pc_expand_step: 14 operations
// per fragment and step for both operands).  The finishing formulas run in the epilogue; every store is a vector store.
// ------------------------------------------------------------------------------------------
struct PairRow {
    static constexpr int NPLANES = 2;
    typedef BpSums<2, true> Sums;                 // n_het, n_hom_alt; wsum
    const u64* rows; size_t row_w64; const u32* weight; u32 snp_begin;
    __device__ void word(u32 i, size_t w, u64 mask, u64 (&v)[2], Sums& sums) const
    {
        const u64* ra = rows + 2 * (size_t)i * row_w64 + w;
        gev_pc_planes(ra[0], ra[row_w64], mask, v[0], v[1]);
        sums.s[0] += gev_pc_popcount64(v[0]); sums.s[1] += gev_pc_popcount64(v[1]);
        if (weight) sums.w += gev_pc_weighted(v[0], v[1], weight, (ptrdiff_t)(64 * w) - (ptrdiff_t)snp_begin);
    }
};
// rows: staged haplotype rows of n_ind individuals (2 per individual, row_w64 words apart), which are individuals [ind_off, +n_ind) of
// the side; the block writes individuals [ind_off, +n_cover) of the planes, zeros beyond n_ind (the pad of the side's last pass).
// planes: n_w4 words x n_pad individuals each or null; weight: n_snps weights (entry j = SNP snp_begin + j) or null; wsum null <=>
// weight null; the three count vectors are indexed like the planes
__global__ void __launch_bounds__(256) k_pair_prep(const u64* __restrict__ rows, size_t row_w64, u32 n_ind, u32 n_cover, u32 ind_off, u32 n_pad,
                                                   u32 snp_begin, u32 n_snps, u32 n_w4,
                                                   u64* __restrict__ plane_x, u64* __restrict__ plane_y, const u32* __restrict__ weight,
                                                   u32* __restrict__ n_het, u32* __restrict__ n_hom, u64* __restrict__ wsum)
{
    bp_prep(PairRow{rows, row_w64, weight, snp_begin}, PairRow::Sums{{0, 0}, 0, {n_het, n_hom}, wsum}, n_ind, n_cover, ind_off, n_pad, snp_begin, n_snps, n_w4, {plane_x, plane_y});
}

struct PairProduct {
    static constexpr int NPLANES = 2, NACC = 2, STEPS = 4;
    __device__ static void expand(const u64 (&w)[2], int s, pc_v4i (&f)[2]) { u32 e[4], g[4]; gev_pc_expand_step(w[0], w[1], s, g, e); f[0] = bp_v4(e); f[1] = bp_v4(g); }   // x, g
};
// planes of side A (n_pad_a individuals) and side B (n_pad_b), n_w4 words each; hom_a / hom_b: n_hom_alt of the n_a / n_b individuals;
// outputs row-major [n_a][n_b], each may be null
template <int FR>
__global__ void __launch_bounds__(256) k_pair_product(const u64* __restrict__ xa_p, const u64* __restrict__ ya_p, u32 n_pad_a,
                                                      const u64* __restrict__ xb_p, const u64* __restrict__ yb_p, u32 n_pad_b, u32 n_w4,
                                                      const u32* __restrict__ hom_a, const u32* __restrict__ hom_b, u32 n_a, u32 n_b,
                                                      u32* __restrict__ n_hethet, u32* __restrict__ n_opphom, u32* __restrict__ dot)
{
    const u64* const pa[2] = {xa_p, ya_p}; const u64* const pb[2] = {xb_p, yb_p};
    u32 a0, b0; pc_v4i acc[2][FR][FR] = {};
    if (!bp_product<FR, PairProduct>(pa, n_pad_a, pb, n_pad_b, n_w4, n_a, n_b, [](u32, u32) { return false; }, a0, b0, acc)) return;
    bp_for_each<FR>(acc, a0, b0, n_a, n_b, [&](u32 i, u32 k, const u32 (&p)[2]) {
        u32 o_hethet, o_opphom, o_dot;
        gev_pc_finish(p[0], p[1], hom_a[i], hom_b[k], o_hethet, o_opphom, o_dot);
        const size_t at = (size_t)i * n_b + k;
        if (n_hethet) n_hethet[at] = o_hethet;
        if (n_opphom) n_opphom[at] = o_opphom;
        if (dot) dot[at] = o_dot;
    });
}
#endif
