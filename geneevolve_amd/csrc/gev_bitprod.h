// gev_bitprod.h -- what the two matrix-core products over bit planes share (gev_paircount.h: pairs of individuals over SNPs;
// gev_ldcount.h: pairs of SNPs over haplotypes).  Both sum, per pair (i of side A, k of side B), a product of small integers over the
// bits of two rows.  A side is prepared into WORD-major bit planes, plane[w * n_pad + row], every word cut to the range of the call
// (gev_pc_range_mask) and padded with zeros to BP_TILE rows and to 4 words -- a zero operand adds nothing to any sum, so the product
// needs no bounds on its loads.  The first part of this file is plain C++ (host and device from one source; any host program can
// include it alone); the device part needs gev_kernels.h (u32, u64).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GEV_PC_HD __host__ __device__
#else
#define GEV_PC_HD
#endif

// the bits of word w (64 w .. 64 w + 63) that lie in [s0, s1)
GEV_PC_HD inline uint64_t gev_pc_range_mask(size_t w, size_t s0, size_t s1)
{
    const size_t lo = w * 64, hi = lo + 64;
    if (s1 <= lo || s0 >= hi || s0 >= s1) return 0;
    uint64_t m = ~(uint64_t)0;
    if (s0 > lo) m &= ~(uint64_t)0 << (s0 - lo);
    if (s1 < hi) m &= ~(uint64_t)0 >> (hi - s1);
    return m;
}
GEV_PC_HD inline uint32_t gev_pc_popcount64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(v);
#else
    return (uint32_t)__builtin_popcountll(v);
#endif
}
// words of a bit row that hold a bit of [begin, +n), padded to the 4 words one product step takes
inline size_t gev_bp_words4(size_t begin, size_t n) { return n ? (((begin + n - 1) >> 6) - (begin >> 6) + 1 + 3) & ~(size_t)3 : 0; }
// the host references keep the operand bytes the device holds in registers: four expanded words = 16 int8 (byte b of word q at 4 q + b)
inline void gev_bp_store16(const uint32_t e[4], int8_t* out)
{
    for (int j = 0; j < 16; j++) out[j] = (int8_t)(e[j >> 2] >> (8 * (j & 3)));
}
// ... and this is their matrix instruction: the i32 accumulator of two rows of operand bytes
inline uint32_t gev_bp_dot_i8(const int8_t* a, const int8_t* b, size_t n)
{
    int32_t acc = 0;
    for (size_t j = 0; j < n; j++) acc += (int32_t)a[j] * b[j];
    return (uint32_t)acc;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// bp_prep: one wave per row of a side walks the words of the range (lane = word, coalesced), writes the row's words into the planes
// and reduces the row's counts over the wave.
//
// bp_product: v_mfma_i32_16x16x64_i8, exact i32 accumulators.  A workgroup of four waves owns a tile of 2 x 2 wave tiles and the whole
// range: no split over the summation index, no atomics.  A wave owns 16 FR x 16 FR pairs = FR x FR fragments of 16 x 16, NACC
// accumulator sets of FR x FR x 4 registers.  Per step of 4 words lane (r = lane & 15, q = lane >> 4) loads ONE word per plane per
// fragment -- word 4 W + q of row r -- straight from the planes (L2; the bit rows are 8x smaller than the operand bytes, and a tile's
// words of a step are shared by the two waves beside it through the cache); the word then feeds P::STEPS matrix steps (P::expand turns
// bits into int8 operand bytes in registers, amortised over the FR fragments of the other side).  Inside a matrix step lane group q
// thus carries the bytes of 16 bits of word 4 W + q in the order the masks give them: a permutation of the summation index that is the
// SAME for the A and the B operand, because both come from the same function of (lane, step), so it cancels in the sum.  What has to
// be right is only the row / column map: A row = lane & 15, B column = lane & 15, C/D column = lane & 15 and row = 4 (lane >> 4) +
// register (bp_for_each).  Every index into the operand and accumulator arrays is a constant once the loops are unrolled.
// ------------------------------------------------------------------------------------------
#define BP_TILE 128u                              // rows the planes are padded to = the larger tile side
typedef int pc_v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ pc_v4i bp_v4(const u32 e[4]) { return pc_v4i{(int)e[0], (int)e[1], (int)e[2], (int)e[3]}; }

// a row's counts: N 32-bit sums and, with W64, a 64-bit one; out / wout: where entry `row` of each goes (each may be null)
template <int N, bool W64> struct BpSums { u32 s[N]; u64 w; u32* out[N]; u64* wout; };
// Row: NPLANES, Sums (a BpSums) and word(row, w, mask, v, sums): word w of row `row` cut to mask into v[NPLANES] and counted.
// The wave's row is row_off + blockIdx.x * 4 + wave of the side: rows [row_off, +n_rows) are read, [row_off, +n_cover) written (zeros
// beyond n_rows: the pad of the side).  plane: n_w4 words x n_pad rows each, or all null; the range is bits [begin, +n) of a row
template <class Row, int N, bool W64>
__device__ __forceinline__ void bp_prep(const Row row, BpSums<N, W64> sums, u32 n_rows, u32 n_cover, u32 row_off, u32 n_pad, u64 begin, u64 n, u32 n_w4,
                                        u64* const (&plane)[Row::NPLANES])
{
    const u32 lane = threadIdx.x & 63u;
    const u32 i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_cover) return;
    const size_t w_first = (size_t)(begin >> 6);
    const u32 n_w = n ? (u32)(((begin + n - 1u) >> 6) - w_first + 1u) : 0u;
    for (u32 w = lane; w < n_w4; w += 64u) {
        u64 v[Row::NPLANES] = {};
        if (i < n_rows && w < n_w) row.word(i, w_first + w, gev_pc_range_mask(w_first + w, (size_t)begin, (size_t)(begin + n)), v, sums);
#pragma unroll
        for (int p = 0; p < Row::NPLANES; p++) if (plane[0]) plane[p][(size_t)w * n_pad + row_off + i] = v[p];
    }
    if (i >= n_rows) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int j = 0; j < N; j++) sums.s[j] += __shfl_xor(sums.s[j], d);
        if (W64) sums.w += __shfl_xor((unsigned long long)sums.w, d);
    }
    if (lane != 0) return;
#pragma unroll
    for (int j = 0; j < N; j++) if (sums.out[j]) sums.out[j][row_off + i] = sums.s[j];
    if (W64 && sums.wout) sums.wout[row_off + i] = sums.w;
}

// P: NPLANES planes per side, NACC accumulator sets, STEPS matrix steps per 64-bit word, expand(words[NPLANES], step, fragments[NACC]).
// pa / pb: the planes of side A (n_pad_a rows) and side B (n_pad_b), n_w4 words each (a multiple of 4).  FR: 16 x 16 fragments per wave
// and side (4: tiles of 128 x 128, 2: tiles of 64 x 64 for blocks too small to fill the device with the large ones).  blockIdx.y = tile
// of A, blockIdx.x = tile of B.  Gives the wave's first pair (a0, b0) and adds its sums to acc[set][m][n] (the caller's, zero at first);
// false: the wave has no pair of [0, n_a) x [0, n_b), or skip(a0, b0) said that none of them is wanted -- nothing was computed
template <int FR, class P, class Skip>
__device__ __forceinline__ bool bp_product(const u64* const (&pa_p)[P::NPLANES], u32 n_pad_a, const u64* const (&pb_p)[P::NPLANES], u32 n_pad_b, u32 n_w4,
                                           u32 n_a, u32 n_b, Skip skip, u32& a0, u32& b0, pc_v4i (&acc)[P::NACC][FR][FR])
{
    constexpr u32 WAVE = 16u * FR, TILE = 2u * WAVE;
    constexpr int NP = P::NPLANES, NACC = P::NACC;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u32 r = lane & 15u, q = lane >> 4;
    a0 = blockIdx.y * TILE + (wave >> 1) * WAVE; b0 = blockIdx.x * TILE + (wave & 1u) * WAVE;
    if (a0 >= n_a || b0 >= n_b || skip(a0, b0)) return false;
    const u64 *pa[NP], *pb[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) { pa[p] = pa_p[p] + (size_t)q * n_pad_a + a0 + r; pb[p] = pb_p[p] + (size_t)q * n_pad_b + b0 + r; }
    struct { u64 a[FR][NP], b[FR][NP]; } cur, next;                   // the step in hand; the next one, loaded while this one is multiplied
    const auto load_next = [&] {
#pragma unroll
        for (int m = 0; m < FR; m++)
#pragma unroll
            for (int p = 0; p < NP; p++) { next.a[m][p] = pa[p][16 * m]; next.b[m][p] = pb[p][16 * m]; }
    };
    load_next();
    for (u32 W = 0; W < n_w4; W += 4u) {
        cur = next;
        if (W + 4u < n_w4) {
#pragma unroll
            for (int p = 0; p < NP; p++) { pa[p] += (size_t)4 * n_pad_a; pb[p] += (size_t)4 * n_pad_b; }
            load_next();
        }
#pragma unroll
        for (int s = 0; s < P::STEPS; s++) {
            pc_v4i fa[FR][NACC], fb[FR][NACC];
#pragma unroll
            for (int m = 0; m < FR; m++) { P::expand(cur.a[m], s, fa[m]); P::expand(cur.b[m], s, fb[m]); }
#pragma unroll
            for (int m = 0; m < FR; m++)
#pragma unroll
                for (int n = 0; n < FR; n++)
#pragma unroll
                    for (int c = 0; c < NACC; c++) acc[c][m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m][c], fb[n][c], acc[c][m][n], 0, 0, 0);
        }
    }
    return true;
}

// the C/D elements of a wave's fragments that lie in [0, n_a) x [0, n_b): f(i, k, values[NACC]).  Column = lane & 15, row =
// 4 (lane >> 4) + register
template <int FR, int NACC, class F>
__device__ __forceinline__ void bp_for_each(const pc_v4i (&acc)[NACC][FR][FR], u32 a0, u32 b0, u32 n_a, u32 n_b, F f)
{
    const u32 lane = threadIdx.x & 63u, r = lane & 15u, q = lane >> 4;
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
                u32 values[NACC];
#pragma unroll
                for (int c = 0; c < NACC; c++) values[c] = (u32)acc[c][m][n][v];
                f(i, k, values);
            }
    }
}
#endif
