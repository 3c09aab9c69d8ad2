// gev_traitsum.h -- per-SNP trait sums from the SNP-major bit rows (gev_snp_trait_sums): what an association scan of the current
// generation is made of.  The reference has no such output; the truth it is held to is numpy over the rows gev_download_haps returns.
//
// A trait is a vector of int32 quanta q[t][i], |q| <= 2^30 (floating-point phenotypes are quantised by the caller), so every sum is
// an integer sum: exact and the same in every order.  Per SNP j and trait t over individuals [ind_begin, +n_ind)
//     gsum[t][j]   = sum_i g_ij q[t][i]                    g = 0/1/2 copies of allele 1                (int64)
//     hetsum[t][j] = sum_{i heterozygous at j} q[t][i]                                                 (int64)
// and the n_het / n_hom_alt of gev_ld_word_counts.  The genotype-class sums follow: S1 = hetsum, S2 = (gsum - hetsum) / 2.
//
// Both are products of SNPs x individuals against individuals x traits on bytes: the digit-column product of gev_digitprod.h with the
// SNPs as rows and the individuals summed (n_ind <= GEV_TS_MAX_IND), the traits its columns.
// Side A is the LD side unchanged (gev_ldcount.h): one plane of masked SNP-major words per block of SNPs; per 32-bit half word
//     genotype bytes      gev_ld_expand_gen                                      byte b of word j = individual 4 b + j, value 0/1/2
//     heterozygote bytes  x = (w ^ w >> 1) & 0x55555555, (x >> 2 j) & 0x01010101   the same order, value 0/1
// Side B in that order: in the step of words 4 W .. 4 W + 3 (counted from the first word of the haplotype range) lane group q carries
// word 4 W + q, matrix step s its half s, and position 4 j + b of the 16 bytes (register j, byte b) holds individual
// 32 (w_first + 4 W + q) + 16 s + 4 b + j -- an individual of the population, not of the range, which need not begin at individual 0
// or on a word.  gev_ts_operand_word is that rule.
//
// The first part of this file is plain C++ (gev_dbg_trait_sums_host and any host program that includes this file alone run the same
// masking, digit split, byte order of both operands and recombination with a plain integer loop in place of the matrix instruction);
// the kernels behind it need gev_kernels.h (u32, u64).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "gev_ldcount.h"                           // gev_ld_word_counts, gev_ld_expand_gen; gev_bitprod.h: the range mask, the words of a range, the byte store
#include "gev_digitprod.h"                         // the digit split, the operand packing, the host product of a row; the epilogue and the finish

#define GEV_TS_MAX_IND GEV_DP_MAX_N               // individuals summed
#define GEV_TS_MAX_Q GEV_DP_MAX_VAL               // |quantum|
#define GEV_TS_SLICE_W 64u                        // words of a SNP's row one workgroup sums: 2048 individuals (a multiple of the 4 words of a step)

// heterozygote bytes of a 32-bit half word (16 individuals), in the order of gev_ld_expand_gen
GEV_PC_HD inline void gev_ts_expand_het(uint32_t w, uint32_t e[4])
{
    const uint32_t x = (w ^ (w >> 1)) & 0x55555555u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) e[j] = (x >> (2 * j)) & 0x01010101u;
}
// Side B: register j of the 16 operand bytes of column `col` of column group `cg` for the half word whose first individual (of the
// population) is i_half: byte b = the column's digit of individual i_half + 4 b + j, 0 outside [ind_begin, +n_ind) and for a trait
// beyond n_traits.  trait: [n_traits][n_ind], entry i = individual ind_begin + i
GEV_PC_HD inline uint32_t gev_ts_operand_word(const int32_t* trait, size_t n_traits, size_t ind_begin, size_t n_ind, size_t i_half, size_t cg, int col, int j)
{
    return gev_dp_operand_word(trait, n_traits, ind_begin, n_ind, cg, col, [=](int b) { return i_half + 4 * (size_t)b + (size_t)j; });
}
// The host form on haplotype-major rows (row r = bits + r * stride words, SNP j = bit j & 63 of word j >> 6): SNPs [snp_begin, +n_snps)
// turned SNP-major over haplotypes [2 ind_begin, +2 n_ind), masked, counted and expanded as the device does; the traits laid out as
// the device's preparation kernel does; gev_bp_dot_i8 in place of the matrix instruction.  Each output may be NULL.  Only the rows of
// the range and, of each, the words that hold a SNP of the range are read
inline void gev_trait_sums_host(const uint64_t* bits, size_t stride, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind,
                                const int32_t* trait, size_t n_traits, int64_t* gsum, int64_t* hetsum, uint32_t* n_het, uint32_t* n_hom_alt)
{
    const size_t h0 = 2 * ind_begin, nh = 2 * n_ind, w_first = h0 >> 6;
    const size_t n_w4 = gev_bp_words4(h0, nh), nb = n_w4 * 32, n_cg = (n_traits + 3) / 4;
    const bool want_sums = (gsum || hetsum) && n_traits;
    std::vector<int8_t> tb;
    if (want_sums) tb = gev_dp_table_host(n_cg, nb, [=](size_t cg, int col, size_t p, int j) { return gev_ts_operand_word(trait, n_traits, ind_begin, n_ind, w_first * 32 + 16 * p, cg, col, j); });
    std::vector<uint64_t> row(n_w4);
    std::vector<int8_t> gb(nb), hb(nb);
    for (size_t s = 0; s < n_snps; s++) {
        const size_t j = snp_begin + s;
        for (size_t w = 0; w < n_w4; w++) row[w] = 0;
        for (size_t h = h0; h < h0 + nh; h++) row[(h >> 6) - w_first] |= ((bits[h * stride + (j >> 6)] >> (j & 63)) & 1ull) << (h & 63);
        uint32_t c = 0, het = 0, hom = 0;
        for (size_t w = 0; w < n_w4; w++) {
            const uint64_t v = row[w] & gev_pc_range_mask(w_first + w, h0, h0 + nh);
            gev_ld_word_counts(v, c, het, hom);
            for (int half = 0; half < 2 && want_sums; half++) {
                const uint32_t w32 = (uint32_t)(v >> (32 * half));
                uint32_t e[4];
                gev_ld_expand_gen(w32, e); gev_bp_store16(e, &gb[w * 32 + 16 * (size_t)half]);
                gev_ts_expand_het(w32, e); gev_bp_store16(e, &hb[w * 32 + 16 * (size_t)half]);
            }
        }
        if (n_het) n_het[s] = het;
        if (n_hom_alt) n_hom_alt[s] = hom;
        if (want_sums) gev_dp_row_host(tb, nb, gb.data(), hb.data(), n_traits, n_snps, s, gsum, hetsum);
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// The device.  Side A: snp_major_device -> k_ld_prep (gev_ldcount.h), as they are.
//
// k_ts_prep: a thread writes the 16 operand bytes (one 16-byte vector store) of one (column group, step, half, lane): the fragment
//   that lane (column lane & 15, word lane >> 4 of the step) of the product loads for that matrix step, so a wave's load of a
//   fragment is 1 KiB in a row.  tb: [column group][n_w4 / 4 steps][2 halves][64 lanes] of 16 bytes.
// k_ts_product: v_mfma_i32_16x16x64_i8, A = 16 SNPs (row = lane & 15), B = the 16 columns of a column group (column = lane & 15),
//   two accumulator sets (genotype bytes, heterozygote bytes).  A block of SNPs against 16 columns is far too few waves, so the
//   individuals are split: blockIdx.x = 128 SNPs (four waves of TS_FR fragments), blockIdx.y = a slice of GEV_TS_SLICE_W words,
//   blockIdx.z = the column group; the partials go to acc through dp_add_partials.  The plane is padded with zero rows to BP_TILE SNPs
//   and to 4 words, tb is whole steps, so no load needs a bound.  acc: [2 sets][n_cg][n_pad SNPs][16 columns].
// The finish is k_dp_finish (gev_digitprod.h).  Every store is a vector one.
// ------------------------------------------------------------------------------------------
#define TS_FR 2                                   // fragments of 16 SNPs a wave: 4 waves x 32 = the BP_TILE SNPs of a workgroup

__global__ void __launch_bounds__(256) k_ts_prep(const int32_t* __restrict__ trait, u32 n_traits, u64 ind_begin, u64 n_ind, u32 n_w4, u32 n_cg, uint4* __restrict__ tb)
{
    const u32 steps = n_w4 >> 2;
    const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (id >= (size_t)n_cg * steps * 128u) return;
    const u32 lane = (u32)id & 63u, s = ((u32)(id >> 6)) & 1u, col = lane & 15u, q = lane >> 4;
    const size_t step = (id >> 7) % steps, cg = (id >> 7) / steps;
    const size_t i_half = ((size_t)((2 * ind_begin) >> 6) + 4 * step + q) * 32 + 16 * s;
    tb[id] = dp_operand16([&](int j) { return gev_ts_operand_word(trait, n_traits, (size_t)ind_begin, (size_t)n_ind, i_half, cg, (int)col, j); });
}

// plane: n_w4 words x n_pad SNPs (k_ld_prep's); cg0: the column group of blockIdx.z = 0
__global__ void __launch_bounds__(256) k_ts_product(const u64* __restrict__ plane, u32 n_pad, u32 n_w4, const uint4* __restrict__ tb, u32 n_cg, u32 cg0, int* __restrict__ acc)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, r = lane & 15u, q = lane >> 4;
    const u32 a0 = blockIdx.x * BP_TILE + wave * 16u * TS_FR;
    const u32 W0 = blockIdx.y * GEV_TS_SLICE_W, W1 = W0 + GEV_TS_SLICE_W < n_w4 ? W0 + GEV_TS_SLICE_W : n_w4;
    const u32 cg = cg0 + blockIdx.z;
    const u64* pa = plane + (size_t)(W0 + q) * n_pad + a0 + r;
    const uint4* pb = tb + ((size_t)cg * (n_w4 >> 2) + (W0 >> 2)) * 128u + lane;
    pc_v4i ag[TS_FR] = {}, ah[TS_FR] = {};
    for (u32 W = W0; W < W1; W += 4u, pa += (size_t)4 * n_pad, pb += 128) {
        u64 a[TS_FR];
#pragma unroll
        for (int m = 0; m < TS_FR; m++) a[m] = pa[16 * m];
        const uint4 b[2] = {pb[0], pb[64]};
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const pc_v4i fb = dp_frag_b(b[s]);
#pragma unroll
            for (int m = 0; m < TS_FR; m++) {
                const u32 w32 = (u32)(a[m] >> (32 * s));
                u32 e[4];
                gev_ld_expand_gen(w32, e); ag[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bp_v4(e), fb, ag[m], 0, 0, 0);
                gev_ts_expand_het(w32, e); ah[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bp_v4(e), fb, ah[m], 0, 0, 0);
            }
        }
    }
    dp_add_partials<TS_FR>(ag, ah, acc, n_cg, n_pad, cg, a0, r, q);
}
#endif
