// gev_identity.h -- identity states per pair of individuals from the ancestry interval lists: the base pairs of a chromosome in each of
// Jacquard's nine condensed identity states (gev_identity_states).  The reference has no such output; the truth it is held to labels
// the elementary intervals of the lists gev_download_intervals returns and looks the pattern of the four labels up in a literal table
// (tests/identity_inputs.py), or labels every position (tools/identity_check.cpp).
//
// f_r(x) is taken as in gev_ibd.h: the (root_population, hap_index) of the part of row r with st <= x < en, labels compared whole,
// undefined where nothing covers x (gaps, rows without parts, parts with st >= en).  New mutations play no part.  For individual i of
// side a (rows 2i, 2i+1 = a0, a1) against individual k of side b (rows 2k, 2k+1 = b0, b1) a position counts only where all four rows
// are covered.  There the equalities among the four labels are a partition of {a0, a1, b0, b1}; as restricted-growth strings in the
// order a0 a1 b0 b1 the 15 partitions are Jacquard's states
//   D1 0000            all four IBD                                   D6 0122            b autozygous, nothing shared
//   D2 0011            each autozygous, different founders            D7 0101 0110       both of a's haplotypes IBD with b's, pairwise
//   D3 0001 0010       a autozygous, shared with one haplotype of b   D8 0102 0120 0112 0121   exactly one pair across
//   D4 0012            a autozygous, b's two distinct, nothing shared D9 0123            nothing shared
//   D5 0100 0111       b autozygous, shared with one haplotype of a
// The result is bp[s][i][k] (u64, plane-major [9][n_a][n_b], plane s - 1 for Ds): the base pairs in state Ds.  Plain 64-bit integers:
// exact and the same bytes on every run.  The nine planes sum to the length along which all four rows are covered; an individual against
// itself is D1 where it is autozygous and D7 elsewhere; swapping the sides swaps D3 with D5 and D4 with D6.
//
// The walk (gev_identity_walk, one source for the device and the host): four cursors; lo = the largest st and hi = the smallest en of the
// four current parts; if lo < hi, hi - lo is added to the state of the four labels; then every list whose part ends at hi moves on, and
// the walk ends when a list is exhausted.  It assumes what the library keeps: along a row neither st nor en decreases and parts do not
// overlap.  Then every part before the one that covers x ends at or before x, so a list is never moved past a position the other three
// have yet to reach, and the overlaps come disjoint and in position order.  A part with st >= en makes lo >= hi for as long as it is
// current and is stepped over like any other.  The four current parts stay in registers; only a list that moved is loaded again.
//
// The first part of this file is plain C++ (gev_dbg_identity_host and any host program that includes this file alone run the same
// walk); the kernel behind it needs gev_kernels.h (u32, u64).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/geneevolve_amd.h"          // gev_part

#if defined(__HIPCC__)
#define GEV_IDN_HD __host__ __device__
#else
#define GEV_IDN_HD
#endif

#define GEV_IDN_TILE 16u                           // individuals a side of a workgroup's tile: 256 pairs, one per lane
#define GEV_IDN_STATES 9u

GEV_IDN_HD inline bool gev_identity_same(const gev_part& x, const gev_part& y) { return x.hap_index == y.hap_index && x.root_population == y.root_population; }
// the state of the four labels, 0 .. 8 for D1 .. D9, without a branch: with both sides autozygous D1 or D2, with one side D3 / D4 or
// D5 / D6 by whether the autozygous label is met on the other side, with neither D7, D8 or D9 by the number of equal pairs across (two
// distinct labels of b cannot both equal one of a's, so that number is at most 2)
GEV_IDN_HD inline uint32_t gev_identity_state(const gev_part& a0, const gev_part& a1, const gev_part& b0, const gev_part& b1)
{
    const uint32_t aa = gev_identity_same(a0, a1), bb = gev_identity_same(b0, b1);
    const uint32_t e00 = gev_identity_same(a0, b0), e01 = gev_identity_same(a0, b1), e10 = gev_identity_same(a1, b0), e11 = gev_identity_same(a1, b1);
    const uint32_t both = 1u - e00;                                  // a0 == a1, b0 == b1: one equality across is all four
    const uint32_t a_only = 3u - (e00 | e01);                        // a0 == a1: shared when either of b's equals it
    const uint32_t b_only = 5u - (e00 | e10);
    const uint32_t neither = 8u - (e00 + e01 + e10 + e11);
    return aa ? (bb ? both : a_only) : (bb ? b_only : neither);
}
// What the walk adds into: add(state, len).  The host keeps nine sums in an array; the kernel's form is further down (GevIdentityLds)
struct GevIdentitySums {
    uint64_t bp[GEV_IDN_STATES];
    GEV_IDN_HD void add(uint32_t s, uint64_t len) { bp[s] += len; }
};
// the pair's sums from the four lists (n0 .. n3 parts; any may be 0: nothing is covered by all four then)
template <class Acc>
GEV_IDN_HD inline void gev_identity_walk(const gev_part* pa0, uint32_t na0, const gev_part* pa1, uint32_t na1,
                                         const gev_part* pb0, uint32_t nb0, const gev_part* pb1, uint32_t nb1, Acc& acc)
{
    if (!na0 || !na1 || !nb0 || !nb1) return;
    uint32_t i0 = 0, i1 = 0, j0 = 0, j1 = 0;
    gev_part A0 = pa0[0], A1 = pa1[0], B0 = pb0[0], B1 = pb1[0];
    for (;;) {
        const uint64_t lo_a = A0.st > A1.st ? A0.st : A1.st, lo_b = B0.st > B1.st ? B0.st : B1.st, lo = lo_a > lo_b ? lo_a : lo_b;
        const uint64_t hi_a = A0.en < A1.en ? A0.en : A1.en, hi_b = B0.en < B1.en ? B0.en : B1.en, hi = hi_a < hi_b ? hi_a : hi_b;
        if (lo < hi) acc.add(gev_identity_state(A0, A1, B0, B1), hi - lo);
        const bool m0 = A0.en <= hi, m1 = A1.en <= hi, m2 = B0.en <= hi, m3 = B1.en <= hi;   // (at least one: hi is one of the four)
        if (m0) { if (++i0 == na0) break; A0 = pa0[i0]; }
        if (m1) { if (++i1 == na1) break; A1 = pa1[i1]; }
        if (m2) { if (++j0 == nb0) break; B0 = pb0[j0]; }
        if (m3) { if (++j1 == nb1) break; B1 = pb1[j1]; }
    }
}
// the host form on lists as gev_download_intervals returns them (n_a, n_b individuals; off_*: 2 n_* + 1 entries): bp [9][n_a][n_b]
inline void gev_identity_host(const gev_part* parts_a, const uint64_t* off_a, size_t n_a, const gev_part* parts_b, const uint64_t* off_b, size_t n_b, uint64_t* bp)
{
    for (size_t i = 0; i < n_a; i++)
        for (size_t k = 0; k < n_b; k++) {
            const gev_part* p[4]; uint32_t n[4];
            for (int h = 0; h < 4; h++) {
                const uint64_t* off = (h < 2 ? off_a + 2 * i : off_b + 2 * k) + (h & 1);
                n[h] = (uint32_t)(off[1] - off[0]);
                p[h] = n[h] ? (h < 2 ? parts_a : parts_b) + off[0] : nullptr;
            }
            GevIdentitySums s = {{0, 0, 0, 0, 0, 0, 0, 0, 0}};
            gev_identity_walk(p[0], n[0], p[1], n[1], p[2], n[2], p[3], n[3], s);
            for (size_t q = 0; q < GEV_IDN_STATES; q++) bp[(q * n_a + i) * n_b + k] = s.bp[q];
        }
}

#if defined(__HIPCC__)
// The kernel's nine sums as [state][lane] words of on-chip memory: 9 x 256 x 8 bytes = 18 KiB a workgroup, so eight workgroups still fit a
// compute unit and no wave is lost; a state's row is 256 words long, so the bank of a word depends on the lane alone and the lanes of a
// wave never meet in one, whatever their states.  An array in registers indexed by the state at run time would go to scratch memory; nine
// sums in registers that every step adds the length or 0 to compile without scratch too, but into 92 registers and 5 waves per SIMD, and
// the whole call was measured 9 to 33 % slower with them
struct GevIdentityLds {
    u64* col;                                                        // this lane's column: col[256 s]
    __device__ void add(u32 s, u64 len) { col[256u * s] += len; }
};
// ------------------------------------------------------------------------------------------
// The device.  k_identity_tiles has the geometry of k_ibd_tiles: a workgroup of 256 threads takes a tile of 16 individuals of side A x 16
// of side B of a sub-block of the pair matrix (blockIdx.y, blockIdx.x), one pair of individuals per lane; wave w takes the 8 x 8 block
// of pairs at (8 (w >> 1), 8 (w & 1)), A individual lane >> 3, B individual lane & 7, so a wave's loads touch 16 + 16 lists.  The lanes
// walk the lists where they lie (read-only loads, a tile's 64 lists stay in the caches).  ind_a, ind_b: the first individuals of the
// sub-block in their populations.  bp: the sub-block's planes [9][n_a][n_b]; every store is a vector store.  No barrier: a lane reads
// and writes its own column of the sums alone.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_identity_tiles(const u32* __restrict__ poff_a, const gev_part* __restrict__ parts_a, u64 ind_a, u32 n_a,
                                                        const u32* __restrict__ poff_b, const gev_part* __restrict__ parts_b, u64 ind_b, u32 n_b,
                                                        u64* __restrict__ bp)
{
    __shared__ u64 sums[GEV_IDN_STATES * 256u];
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const u32 ia = blockIdx.y * GEV_IDN_TILE + 8u * (wave >> 1) + (lane >> 3), ib = blockIdx.x * GEV_IDN_TILE + 8u * (wave & 1u) + (lane & 7u);
    if (ia >= n_a || ib >= n_b) return;
    const u32* oa = poff_a + 2 * (ind_a + ia); const u32* ob = poff_b + 2 * (ind_b + ib);
    const u32 a0 = oa[0], a1 = oa[1], a2 = oa[2], b0 = ob[0], b1 = ob[1], b2 = ob[2];
    const size_t o = (size_t)ia * n_b + ib, plane = (size_t)n_a * n_b;
    GevIdentityLds acc = {sums + threadIdx.x};
#pragma unroll
    for (u32 q = 0; q < GEV_IDN_STATES; q++) acc.col[256u * q] = 0;
    gev_identity_walk(parts_a + a0, a1 - a0, parts_a + a1, a2 - a1, parts_b + b0, b1 - b0, parts_b + b1, b2 - b1, acc);
#pragma unroll
    for (u32 q = 0; q < GEV_IDN_STATES; q++) bp[q * plane + o] = acc.col[256u * q];
}
#endif
