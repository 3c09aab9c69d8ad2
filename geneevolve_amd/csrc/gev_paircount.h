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
// at a time.  The order of the loci inside a step is free as long as both operands of a product use the same one -- a permutation of
// the summation index cancels in the sum -- so the loci are taken where masks alone find them.  Of a 32-locus half word the loci of one
// parity are packed as 2-bit fields (gev_pc_pack2)
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

#if defined(__HIPCC__)
#define GEV_PC_HD __host__ __device__
#else
#define GEV_PC_HD
#endif

#define GEV_PC_MAX_SNPS ((size_t)1 << 30)         // dot can reach 4 * n_snps

// the loci of word w (64 w .. 64 w + 63) that lie in [s0, s1)
GEV_PC_HD inline uint64_t gev_pc_range_mask(size_t w, size_t s0, size_t s1)
{
    const size_t lo = w * 64, hi = lo + 64;
    if (s1 <= lo || s0 >= hi || s0 >= s1) return 0;
    uint64_t m = ~(uint64_t)0;
    if (s0 > lo) m &= ~(uint64_t)0 << (s0 - lo);
    if (s1 < hi) m &= ~(uint64_t)0 >> (hi - s1);
    return m;
}
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
GEV_PC_HD inline uint32_t gev_pc_popcount64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(v);
#else
    return (uint32_t)__builtin_popcountll(v);
#endif
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
                for (int q = 0; q < 4; q++)
                    for (int b = 0; b < 4; b++) {
                        xb[i * n_bytes + w * 64 + 16 * s + 4 * q + b] = (int8_t)(xe[q] >> (8 * b));
                        gb[i * n_bytes + w * 64 + 16 * s + 4 * q + b] = (int8_t)(ge[q] >> (8 * b));
                    }
            }
        }
        if (n_het) n_het[i] = het[i];
        if (n_hom_alt) n_hom_alt[i] = hom[i];
    }
    if (!n_hethet && !n_opphom && !dot) return;
    for (size_t i = 0; i < n_a; i++)
        for (size_t k = 0; k < n_b; k++) {
            const int8_t* xi = xb.data() + (a_begin + i) * n_bytes; const int8_t* xk = xb.data() + (b_begin + k) * n_bytes;
            const int8_t* gi = gb.data() + (a_begin + i) * n_bytes; const int8_t* gk = gb.data() + (b_begin + k) * n_bytes;
            int32_t xx = 0, gg = 0;                                  // the accumulators of the matrix instruction
            for (size_t j = 0; j < n_bytes; j++) { xx += (int32_t)xi[j] * xk[j]; gg += (int32_t)gi[j] * gk[j]; }
            uint32_t o_hethet, o_opphom, o_dot;
            gev_pc_finish((uint32_t)xx, (uint32_t)gg, hom[a_begin + i], hom[b_begin + k], o_hethet, o_opphom, o_dot);
            if (n_hethet) n_hethet[i * n_b + k] = o_hethet;
            if (n_opphom) n_opphom[i * n_b + k] = o_opphom;
            if (dot) dot[i * n_b + k] = o_dot;
        }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// The device.  Both kernels read STAGED rows (stage_rows_mutated: pool units resolved, mutation overlay applied, once per row).
//
// 1. k_pair_prep: one wave per individual walks the words of the SNP range (lane = word, coalesced), writes the individual's x and y
// words into the two planes and reduces n_het, n_hom_alt and, with weights, wsum over the wave.  The planes are WORD-major:
// plane[w * n_pad + i], so that the product's 16 lanes of a fragment row read 16 consecutive words.  They are padded to PC_TILE
// individuals and to 4 words with zeros (a zero operand adds nothing to any sum), so the product needs no bounds on its loads.
// gev_ind_genotype_counts is this kernel alone, without planes.
//
// 2. k_pair_product: v_mfma_i32_16x16x64_i8, exact i32 accumulators.  A workgroup of four waves owns a PC_TILE x PC_TILE tile of pairs
// and the whole SNP range: no split over the loci, no atomics.  A wave owns 64 x 64 pairs = 4 x 4 fragments of 16 x 16, two accumulator
// sets (xx, gg) of 16 x 4 registers each.  Per step of 256 loci lane (r = lane & 15, q = lane >> 4) loads ONE word per plane per
// fragment -- word 4 W + q of individual r -- straight from the planes (L2; the bit rows are 8x smaller than the operand bytes, and a
// tile's 2 x 128 x 2 words of a step are shared by the two waves beside it through the cache); the word then feeds four matrix steps
// (gev_pc_expand_step).  Inside a matrix step lane group q thus carries 16 loci of word 4 W + q in the order the masks give them: a
// permutation of the k index that is the SAME for the A and the B operand, because both come from the same function of (lane, step),
// so it cancels in the sum over k.  What has to be right is only the row / column map: A row = lane & 15, B column = lane & 15,
// C/D column = lane & 15 and row = 4 (lane >> 4) + register.  The expansion (14 operations per fragment and step for both operands) is
// amortised over the 4 fragments of the other side.  The finishing formulas run in the epilogue; every store is a vector store.
// ------------------------------------------------------------------------------------------
#define PC_TILE 128u                              // individuals the planes are padded to = the larger tile side
typedef int pc_v4i __attribute__((ext_vector_type(4)));

// rows: staged haplotype rows of n_ind individuals (2 per individual, row_w64 words apart), which are individuals [ind_off, +n_ind) of
// the side; the block writes individuals [ind_off, +n_cover) of the planes, zeros beyond n_ind (the pad of the side's last pass).
// planes: n_w4 words x n_pad individuals each or null; weight: n_snps weights (entry j = SNP snp_begin + j) or null; wsum null <=>
// weight null; the three count vectors are indexed like the planes
__global__ void __launch_bounds__(256) k_pair_prep(const u64* __restrict__ rows, size_t row_w64, u32 n_ind, u32 n_cover, u32 ind_off, u32 n_pad,
                                                   u32 snp_begin, u32 n_snps, u32 n_w4,
                                                   u64* __restrict__ plane_x, u64* __restrict__ plane_y, const u32* __restrict__ weight,
                                                   u32* __restrict__ n_het, u32* __restrict__ n_hom, u64* __restrict__ wsum)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_cover) return;
    const u32 snp_end = snp_begin + n_snps, w_first = snp_begin >> 6;
    const u32 n_w = n_snps ? ((snp_end - 1u) >> 6) - w_first + 1u : 0u;
    u32 het = 0, hom = 0; u64 ws = 0;
    for (u32 w = lane; w < n_w4; w += 64u) {
        u64 x = 0, y = 0;
        if (i < n_ind && w < n_w) {
            const u64* ra = rows + 2 * (size_t)i * row_w64 + w_first + w;
            gev_pc_planes(ra[0], ra[row_w64], gev_pc_range_mask(w_first + w, snp_begin, snp_end), x, y);
            het += gev_pc_popcount64(x); hom += gev_pc_popcount64(y);
            if (weight) ws += gev_pc_weighted(x, y, weight, (ptrdiff_t)64 * (w_first + w) - (ptrdiff_t)snp_begin);
        }
        if (plane_x) { plane_x[(size_t)w * n_pad + ind_off + i] = x; plane_y[(size_t)w * n_pad + ind_off + i] = y; }
    }
    if (i >= n_ind) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { het += __shfl_xor(het, d); hom += __shfl_xor(hom, d); ws += __shfl_xor((unsigned long long)ws, d); }
    if (lane == 0) {
        if (n_het) n_het[ind_off + i] = het;
        if (n_hom) n_hom[ind_off + i] = hom;
        if (wsum) wsum[ind_off + i] = ws;
    }
}

// planes of side A (n_pad_a individuals) and side B (n_pad_b), n_w4 words each (a multiple of 4); hom_a / hom_b: n_hom_alt of the n_a / n_b
// individuals; outputs row-major [n_a][n_b], each may be null.  FR: 16 x 16 fragments per wave and side (4: tiles of 128 x 128, 2: tiles of
// 64 x 64 for blocks too small to fill the device with the large ones).  blockIdx.y = tile of A, blockIdx.x = tile of B
template <int FR>
__global__ void __launch_bounds__(256) k_pair_product(const u64* __restrict__ xa_p, const u64* __restrict__ ya_p, u32 n_pad_a,
                                                      const u64* __restrict__ xb_p, const u64* __restrict__ yb_p, u32 n_pad_b, u32 n_w4,
                                                      const u32* __restrict__ hom_a, const u32* __restrict__ hom_b, u32 n_a, u32 n_b,
                                                      u32* __restrict__ n_hethet, u32* __restrict__ n_opphom, u32* __restrict__ dot)
{
    constexpr u32 WAVE = 16u * FR, TILE = 2u * WAVE;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u32 r = lane & 15u, q = lane >> 4;
    const u32 a0 = blockIdx.y * TILE + (wave >> 1) * WAVE, b0 = blockIdx.x * TILE + (wave & 1u) * WAVE;         // the wave's pairs
    if (a0 >= n_a || b0 >= n_b) return;                                                                        // (nothing of the wave's is stored)
    pc_v4i acc_x[FR][FR], acc_g[FR][FR];
#pragma unroll
    for (int m = 0; m < FR; m++)
#pragma unroll
        for (int n = 0; n < FR; n++) { acc_x[m][n] = pc_v4i{0, 0, 0, 0}; acc_g[m][n] = pc_v4i{0, 0, 0, 0}; }
    const u64* pxa = xa_p + (size_t)q * n_pad_a + a0 + r; const u64* pya = ya_p + (size_t)q * n_pad_a + a0 + r;
    const u64* pxb = xb_p + (size_t)q * n_pad_b + b0 + r; const u64* pyb = yb_p + (size_t)q * n_pad_b + b0 + r;
    u64 xa[FR], ya[FR], xb[FR], yb[FR];                       // the step in hand
    u64 nxa[FR], nya[FR], nxb[FR], nyb[FR];                   // the next one, loaded while this one is multiplied
#pragma unroll
    for (int m = 0; m < FR; m++) { nxa[m] = pxa[16 * m]; nya[m] = pya[16 * m]; nxb[m] = pxb[16 * m]; nyb[m] = pyb[16 * m]; }
    for (u32 W = 0; W < n_w4; W += 4u) {
#pragma unroll
        for (int m = 0; m < FR; m++) { xa[m] = nxa[m]; ya[m] = nya[m]; xb[m] = nxb[m]; yb[m] = nyb[m]; }
        if (W + 4u < n_w4) {
            pxa += (size_t)4 * n_pad_a; pya += (size_t)4 * n_pad_a; pxb += (size_t)4 * n_pad_b; pyb += (size_t)4 * n_pad_b;
#pragma unroll
            for (int m = 0; m < FR; m++) { nxa[m] = pxa[16 * m]; nya[m] = pya[16 * m]; nxb[m] = pxb[16 * m]; nyb[m] = pyb[16 * m]; }
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            pc_v4i ax[FR], ag[FR], bx[FR], bg[FR];
#pragma unroll
            for (int m = 0; m < FR; m++) {
                u32 e[4], g[4];
                gev_pc_expand_step(xa[m], ya[m], s, g, e);
                ax[m] = pc_v4i{(int)e[0], (int)e[1], (int)e[2], (int)e[3]}; ag[m] = pc_v4i{(int)g[0], (int)g[1], (int)g[2], (int)g[3]};
                gev_pc_expand_step(xb[m], yb[m], s, g, e);
                bx[m] = pc_v4i{(int)e[0], (int)e[1], (int)e[2], (int)e[3]}; bg[m] = pc_v4i{(int)g[0], (int)g[1], (int)g[2], (int)g[3]};
            }
#pragma unroll
            for (int m = 0; m < FR; m++)
#pragma unroll
                for (int n = 0; n < FR; n++) {
                    acc_x[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ax[m], bx[n], acc_x[m][n], 0, 0, 0);
                    acc_g[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag[m], bg[n], acc_g[m][n], 0, 0, 0);
                }
        }
    }
    // C/D: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int n = 0; n < FR; n++) {
        const u32 k = b0 + 16u * n + r;
        if (k >= n_b) continue;
        const u32 hk = hom_b[k];
#pragma unroll
        for (int m = 0; m < FR; m++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const u32 i = a0 + 16u * m + 4u * q + v;
                if (i >= n_a) continue;
                u32 o_hethet, o_opphom, o_dot;
                gev_pc_finish((u32)acc_x[m][n][v], (u32)acc_g[m][n][v], hom_a[i], hk, o_hethet, o_opphom, o_dot);
                const size_t at = (size_t)i * n_b + k;
                if (n_hethet) n_hethet[at] = o_hethet;
                if (n_opphom) n_opphom[at] = o_opphom;
                if (dot) dot[at] = o_dot;
            }
    }
}
#endif
