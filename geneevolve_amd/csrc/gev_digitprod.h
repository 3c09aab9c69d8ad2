// gev_digitprod.h -- the signed digit-column product under gev_snp_trait_sums (G^T Y, gev_traitsum.h) and gev_ind_scores (G W,
// gev_indscore.h): what the two share and nothing that knows which axis of the genotype matrix is summed.
//
// Side A are rows of genotype bytes (0/1/2) and heterozygote bytes (0/1) expanded from bit planes; side B are host columns of int32
// values, |v| <= 2^30, each split into four balanced base-256 digits in [-128, 127] (v = sum_k d_k 256^k; the last one is what is left,
// |d_3| <= 65).  4 columns x 4 digits = the 16 columns of one v_mfma_i32_16x16x64_i8 fragment: column 4 (t & 3) + k of column group
// t >> 2.  The accumulators are i32: |digit| <= 128, g <= 2, so 2^22 summed entries keep them within 2^30; sum_k acc_k 256^k is formed
// in 64 bits, |sum| <= 2^53.  Unlike gev_bitprod.h's products, whose operands come from one function of (lane, step), side B is made
// elsewhere than side A, so its bytes lie in exactly the order the expansion gives side A's: which summed entry byte b of register j
// names is the one thing a feature states (gev_ts_operand_word, gev_is_operand_word).
//
// The first part of this file is plain C++, for the host forms of the two features; the device part needs gev_kernels.h (u32).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "gev_bitprod.h"                           // GEV_PC_HD, the byte store and dot; on the device pc_v4i

#define GEV_DP_MAX_N ((size_t)1 << 22)            // summed entries of a row: 128 * 2 * 2^22 = 2^30, an accumulator stays an int32
#define GEV_DP_MAX_VAL ((int32_t)1 << 30)         // |value|

// balanced base-256 digit k (0..3) of a value: v = d0 + 256 d1 + 256^2 d2 + 256^3 d3, d0..d2 in [-128, 127]
GEV_PC_HD inline int32_t gev_dp_digit(int32_t v, int k)
{
    int32_t d = 0;
    for (int i = 0; i <= k; i++) { d = ((v + 128) & 255) - 128; v = (v - d) / 256; }
    return d;
}
// sum_k acc[k] 256^k
GEV_PC_HD inline int64_t gev_dp_recombine(const int32_t acc[4])
{
    return (int64_t)acc[0] + (int64_t)acc[1] * 256 + (int64_t)acc[2] * 65536 + (int64_t)acc[3] * 16777216;
}
// One register of the 16 operand bytes of column `col` of column group `cg`: byte b = the column's digit of summed entry index(b) (counted
// on the whole axis), 0 outside [begin, +n) and for a column beyond n_cols.  val: [n_cols][n], entry i = entry begin + i of the axis
template <class Index>
GEV_PC_HD inline uint32_t gev_dp_operand_word(const int32_t* val, size_t n_cols, size_t begin, size_t n, size_t cg, int col, Index index)
{
    const size_t t = 4 * cg + (size_t)(col >> 2);
    if (t >= n_cols) return 0;
    uint32_t r = 0;
    for (int b = 0; b < 4; b++) {
        const size_t i = index(b);
        if (i >= begin && i - begin < n) r |= (uint32_t)(uint8_t)gev_dp_digit(val[t * n + (i - begin)], col & 3) << (8 * b);
    }
    return r;
}
// The host's side B: [column group][column][the nb bytes of a row], laid out as a feature's preparation kernel does.  word(cg, col, p, j) is
// the feature's operand rule for register j of the p-th run of 16 bytes
template <class Word>
inline std::vector<int8_t> gev_dp_table_host(size_t n_cg, size_t nb, Word word)
{
    std::vector<int8_t> tb(n_cg * 16 * nb);
    for (size_t cg = 0; cg < n_cg; cg++)
        for (int col = 0; col < 16; col++)
            for (size_t p = 0; p < nb / 16; p++) {
                uint32_t e[4];
                for (int j = 0; j < 4; j++) e[j] = word(cg, col, p, j);
                gev_bp_store16(e, &tb[(cg * 16 + (size_t)col) * nb + 16 * p]);
            }
    return tb;
}
// One row of the host's product: its genotype bytes gb and heterozygote bytes hb against every column of tb, gev_bp_dot_i8 in place of the
// matrix instruction, into gout / hout [n_cols][n] at `row` (each may be NULL)
inline void gev_dp_row_host(const std::vector<int8_t>& tb, size_t nb, const int8_t* gb, const int8_t* hb, size_t n_cols, size_t n, size_t row, int64_t* gout, int64_t* hout)
{
    for (size_t t = 0; t < n_cols; t++) {
        int32_t ag[4], ah[4];
        for (int k = 0; k < 4; k++) {
            const int8_t* b = &tb[((t >> 2) * 16 + 4 * (t & 3) + (size_t)k) * nb];
            ag[k] = (int32_t)gev_bp_dot_i8(gb, b, nb); ah[k] = (int32_t)gev_bp_dot_i8(hb, b, nb);
        }
        if (gout) gout[t * n + row] = gev_dp_recombine(ag);
        if (hout) hout[t * n + row] = gev_dp_recombine(ah);
    }
}

#if defined(__HIPCC__)
// The device.  A feature's product kernel keeps two accumulator sets (genotype bytes, heterozygote bytes) per fragment of 16 rows and adds
// its i32 partials with vector atomics (integer adds commute; two's-complement wrap is harmless while the total is in range) into
// acc: [2 sets][n_cg][n_pad rows][16 columns]; a zero partial is not added.  Every store and atomic is a vector one.

// the 16 operand bytes a thread of a preparation kernel stores: register j = word(j), a feature's operand rule
template <class Word> __device__ __forceinline__ uint4 dp_operand16(Word word) { return make_uint4(word(0), word(1), word(2), word(3)); }
// fragment B of a matrix step from those 16 bytes
__device__ __forceinline__ pc_v4i dp_frag_b(const uint4& b) { return pc_v4i{(int)b.x, (int)b.y, (int)b.z, (int)b.w}; }
// a wave's FR fragments (rows a0 .. a0 + 16 FR - 1 against column group cg) added to acc by lane (r, q) = (lane & 15, lane >> 4).  C/D: column = r, row = 4 q + register
template <int FR>
__device__ __forceinline__ void dp_add_partials(const pc_v4i (&ag)[FR], const pc_v4i (&ah)[FR], int* acc, u32 n_cg, u32 n_pad, u32 cg, u32 a0, u32 r, u32 q)
{
    int* const og = acc + ((size_t)cg * n_pad + a0) * 16u + r;
    int* const oh = og + (size_t)n_cg * n_pad * 16u;
#pragma unroll
    for (int m = 0; m < FR; m++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const size_t o = (size_t)(16 * m + 4 * (int)q + v) * 16u;
            if (ag[m][v]) atomicAdd(og + o, ag[m][v]);
            if (ah[m][v]) atomicAdd(oh + o, ah[m][v]);
        }
}

// sum_k acc_k 256^k per (column, row) in 64 bits, out: [2 sets][n_cols][out_stride rows]
__global__ void __launch_bounds__(256) k_dp_finish(const int* __restrict__ acc, u32 n_pad, u32 n_cg, u32 n_cols, u32 n, u32 out_stride, long long* __restrict__ out)
{
    const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (id >= (size_t)2 * n_cols * n) return;
    const u32 j = (u32)(id % n), t = (u32)((id / n) % n_cols), set = (u32)(id / ((size_t)n * n_cols));
    const int4 a = *(const int4*)(acc + (((size_t)set * n_cg + (t >> 2)) * n_pad + j) * 16u + 4u * (t & 3u));
    const int32_t d[4] = {a.x, a.y, a.z, a.w};
    out[((size_t)set * n_cols + t) * out_stride + j] = gev_dp_recombine(d);
}
#endif
