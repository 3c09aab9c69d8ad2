// gev_indscore.h -- per-individual scores from the haplotype-major bit rows (gev_ind_scores): G W, individuals x SNPs against SNPs x
// weight columns -- polygenic scores with signed effect sizes, several dozen columns in one pass, and with gev_snp_trait_sums (G^T Y)
// the two products a randomised subspace iteration for the principal components needs.  The reference has no such output; the truth
// it is held to is numpy over the rows gev_download_haps returns.
//
// A score column is a host vector of int32 weights w[s][j], |w| <= 2^30 (floating-point effect sizes are quantised by the caller), so
// every sum is an integer sum: exact and the same in every order.  Per individual i and column s over SNPs [snp_begin, +n_snps)
//     gscore[s][i]   = sum_j w[s][j] g_ij                    g = 0/1/2 copies of allele 1                (int64)
//     hetscore[s][i] = sum_{j : i heterozygous at j} w[s][j]                                             (int64)
// The genotype-class sums follow: S1 = hetscore, S2 = (gscore - hetscore) / 2.  Both are additive over SNP ranges and chromosomes.
//
// Both are products of individuals x SNPs against SNPs x columns on bytes.
// Side A is the pair side unchanged (gev_paircount.h): the range-masked individual-major planes x = a ^ b and y = a & b, and per
// matrix step of a 64-locus word gev_pc_expand_step gives the genotype bytes (x + 2y) and the heterozygote bytes (x).
// Side B are the weights: the digit-column product of gev_digitprod.h with the individuals as rows and the SNPs summed (n_snps <=
// GEV_IS_MAX_SNPS), the score columns its columns.  Its bytes in side A's order: in the step of words 4 W .. 4 W + 3 (counted from the
// first word of the SNP range) lane group q carries word 4 W + q; of that word matrix step s (0..3) takes the loci of half s >> 1 and
// parity s & 1 (gev_pc_pack2: field f = locus 2 f + parity of the half), and position 4 j + b of the 16 bytes (register j, byte b) holds
// field j + 4 b (gev_pc_expand), that is SNP
//     64 (w_first + 4 W + q) + 32 (s >> 1) + 2 (j + 4 b) + (s & 1)
// of the chromosome.  gev_is_operand_word is that rule.
//
// The first part of this file is plain C++ (gev_dbg_ind_scores_host and any host program that includes this file alone run the same
// masking, digit split, byte order of both operands and recombination with a plain integer loop in place of the matrix instruction);
// the kernels behind it need gev_kernels.h (u32, u64).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "gev_paircount.h"                         // gev_pc_planes, gev_pc_expand_step; gev_bitprod.h: the range mask, the words of a range, the byte store
#include "gev_digitprod.h"                         // the digit split, the operand packing, the host product of a row; the epilogue and the finish

#define GEV_IS_MAX_SNPS GEV_DP_MAX_N              // SNPs summed
#define GEV_IS_MAX_W GEV_DP_MAX_VAL               // |weight|
#define GEV_IS_SLICE_W 64u                        // words of an individual's planes one workgroup sums: 4096 SNPs (a multiple of the 4 words of a step)

// Side B: register j of the 16 operand bytes of column `col` of column group `cg` for matrix step s (0..3) of word `word` of the
// chromosome: byte b = the column's digit of SNP 64 word + 32 (s >> 1) + 2 (j + 4 b) + (s & 1), 0 outside [snp_begin, +n_snps) and
// for a column beyond n_scores.  weight: [n_scores][n_snps], entry j = SNP snp_begin + j
GEV_PC_HD inline uint32_t gev_is_operand_word(const int32_t* weight, size_t n_scores, size_t snp_begin, size_t n_snps, size_t word, int s, size_t cg, int col, int j)
{
    return gev_dp_operand_word(weight, n_scores, snp_begin, n_snps, cg, col, [=](int b) { return 64 * word + 32 * (size_t)(s >> 1) + 2 * (size_t)(j + 4 * b) + (size_t)(s & 1); });
}
// The host form on haplotype-major rows (row r = bits + r * stride words, SNP j = bit j & 63 of word j >> 6, rows 2i and 2i+1 =
// individual i): the planes of individuals [ind_begin, +n_ind) masked and expanded as the device does; the weights laid out as the
// device's preparation kernel does; gev_bp_dot_i8 in place of the matrix instruction.  Each output may be NULL.  Only the rows of the
// range and, of each, the words that hold a SNP of the range are read
inline void gev_ind_scores_host(const uint64_t* bits, size_t stride, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind,
                                const int32_t* weight, size_t n_scores, int64_t* gscore, int64_t* hetscore)
{
    const size_t snp_end = snp_begin + n_snps, w_first = snp_begin >> 6;
    const size_t n_w = n_snps ? ((snp_end - 1) >> 6) - w_first + 1 : 0, n_w4 = gev_bp_words4(snp_begin, n_snps);
    const size_t nb = n_w4 * 64, n_cg = (n_scores + 3) / 4;
    if ((!gscore && !hetscore) || !n_scores) return;
    const std::vector<int8_t> tb = gev_dp_table_host(n_cg, nb, [=](size_t cg, int col, size_t p, int j) { return gev_is_operand_word(weight, n_scores, snp_begin, n_snps, w_first + (p >> 2), (int)(p & 3), cg, col, j); });
    std::vector<int8_t> gb(nb), hb(nb);
    for (size_t i = 0; i < n_ind; i++) {
        const uint64_t* ra = bits + 2 * (ind_begin + i) * stride; const uint64_t* rb = ra + stride;
        for (size_t w = 0; w < n_w4; w++) {
            uint64_t x = 0, y = 0;
            if (w < n_w) gev_pc_planes(ra[w_first + w], rb[w_first + w], gev_pc_range_mask(w_first + w, snp_begin, snp_end), x, y);
            for (int s = 0; s < 4; s++) {
                uint32_t xe[4], ge[4];
                gev_pc_expand_step(x, y, s, ge, xe);
                gev_bp_store16(ge, &gb[w * 64 + 16 * (size_t)s]); gev_bp_store16(xe, &hb[w * 64 + 16 * (size_t)s]);
            }
        }
        gev_dp_row_host(tb, nb, gb.data(), hb.data(), n_scores, n_ind, i, gscore, hetscore);
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// The device.  Side A: pair_prep_side -> k_pair_prep (gev_paircount.h), as they are.
//
// k_is_prep: a thread writes the 16 operand bytes (one 16-byte vector store) of one (column group, step of 4 words, matrix step,
//   lane): the fragment that lane (column lane & 15, word lane >> 4 of the step) of the product loads for that matrix step, so a
//   wave's load of a fragment is 1 KiB in a row.  tb: [column group][n_w4 / 4 steps][4 matrix steps][64 lanes] of 16 bytes.
// k_is_product: v_mfma_i32_16x16x64_i8, A = 16 individuals (row = lane & 15), B = the 16 columns of a column group (column =
//   lane & 15), two accumulator sets (genotype bytes, heterozygote bytes).  The SNPs are split so that a block of individuals against
//   16 columns fills the device: blockIdx.x = 128 individuals (four waves of IS_FR fragments), blockIdx.y = a slice of
//   GEV_IS_SLICE_W words, blockIdx.z = the column group; the partials go to acc through dp_add_partials.  The planes are padded with
//   zero individuals to BP_TILE and to 4 words, tb is whole steps, so no load needs a bound.  The next step's words and fragments are
//   loaded before this step's products are issued.  acc: [2 sets][n_cg][n_pad individuals][16 columns].
// The finish is k_dp_finish (gev_digitprod.h).  Every store is a vector one.
// ------------------------------------------------------------------------------------------
#define IS_FR 2                                   // fragments of 16 individuals a wave: 4 waves x 32 = the BP_TILE individuals of a workgroup

__global__ void __launch_bounds__(256) k_is_prep(const int32_t* __restrict__ weight, u32 n_scores, u64 snp_begin, u64 n_snps, u32 n_w4, u32 n_cg, uint4* __restrict__ tb)
{
    const u32 steps = n_w4 >> 2;
    const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (id >= (size_t)n_cg * steps * 256u) return;
    const u32 lane = (u32)id & 63u, s = ((u32)(id >> 6)) & 3u, col = lane & 15u, q = lane >> 4;
    const size_t step = (id >> 8) % steps, cg = (id >> 8) / steps;
    const size_t word = (size_t)(snp_begin >> 6) + 4 * step + q;
    tb[id] = dp_operand16([&](int j) { return gev_is_operand_word(weight, n_scores, (size_t)snp_begin, (size_t)n_snps, word, (int)s, cg, (int)col, j); });
}

// plane_x / plane_y: n_w4 words x n_pad individuals each (k_pair_prep's); cg0: the column group of blockIdx.z = 0
__global__ void __launch_bounds__(256) k_is_product(const u64* __restrict__ plane_x, const u64* __restrict__ plane_y, u32 n_pad, u32 n_w4,
                                                    const uint4* __restrict__ tb, u32 n_cg, u32 cg0, int* __restrict__ acc)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, r = lane & 15u, q = lane >> 4;
    const u32 a0 = blockIdx.x * BP_TILE + wave * 16u * IS_FR;
    const u32 W0 = blockIdx.y * GEV_IS_SLICE_W, W1 = W0 + GEV_IS_SLICE_W < n_w4 ? W0 + GEV_IS_SLICE_W : n_w4;
    const u32 cg = cg0 + blockIdx.z;
    const u64* px = plane_x + (size_t)(W0 + q) * n_pad + a0 + r;
    const u64* py = plane_y + (size_t)(W0 + q) * n_pad + a0 + r;
    const uint4* pb = tb + ((size_t)cg * (n_w4 >> 2) + (W0 >> 2)) * 256u + lane;
    struct { u64 x[IS_FR], y[IS_FR]; uint4 b[4]; } cur, next;       // the step in hand; the next one, loaded while this one is multiplied
    const auto load_next = [&] {
#pragma unroll
        for (int m = 0; m < IS_FR; m++) { next.x[m] = px[16 * m]; next.y[m] = py[16 * m]; }
#pragma unroll
        for (int s = 0; s < 4; s++) next.b[s] = pb[64 * s];
    };
    pc_v4i ag[IS_FR] = {}, ah[IS_FR] = {};
    load_next();
    for (u32 W = W0; W < W1; W += 4u) {
        cur = next;
        if (W + 4u < W1) { px += (size_t)4 * n_pad; py += (size_t)4 * n_pad; pb += 256; load_next(); }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const pc_v4i fb = dp_frag_b(cur.b[s]);
#pragma unroll
            for (int m = 0; m < IS_FR; m++) {
                u32 g[4], e[4];
                gev_pc_expand_step(cur.x[m], cur.y[m], s, g, e);
                ag[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bp_v4(g), fb, ag[m], 0, 0, 0);
                ah[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bp_v4(e), fb, ah[m], 0, 0, 0);
            }
        }
    }
    dp_add_partials<IS_FR>(ag, ah, acc, n_cg, n_pad, cg, a0, r, q);
}
#endif
