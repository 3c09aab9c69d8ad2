// gev_lineage.h -- founder lineages along the genome from the ancestry interval lists: the founder every haplotype row descends from at
// given positions (gev_founder_at) and, per position, the rows by founder with their summary (gev_founder_counts).  The reference has no
// such output; the truth it is held to is a linear scan per (row, position) of the lists gev_download_intervals returns
// (tests/lineage_inputs.py, tools/lineage_check.cpp).
//
// A row's list is what the library keeps for it: gev_part records in position order, half-open [st, en), no two overlapping; st and en
// each do not decrease along the row (gaps, rows without parts and parts with st >= en, which cover nothing, are allowed).  f_r(x) =
// (root_population, hap_index) of the part of row r with st <= x < en, as in gev_ibd.h; undefined where no part covers x: in a gap, in a
// row without parts, before the first part, at or behind the last en.  New mutations play no part.  With n_founder_haps[n_pop] founder
// haplotypes per root population, base[p] their exclusive prefix sum and F their total, the FOUNDER ID of a covered position is fid =
// base[root_population] + hap_index (u32, F <= 2^32 - 2) and GEV_NO_FOUNDER (2^32 - 1) marks an uncovered one.  Per position over the rows
// of a range: counts[f] = the rows with founder id f, and the site record n_covered = sum counts, n_lineages = the f with counts[f] != 0,
// sum_sq = sum counts^2, top_count = max counts, top_founder = the LOWEST f with counts[f] == top_count (GEV_NO_FOUNDER when n_covered is
// 0); pop_counts[p] = the rows whose covering part has root population p = the sum of counts over [base[p], base[p + 1]).  Plain
// integers: exact and the same on every run.
//
// The walk (one source for the device and the host): positions come in non-decreasing order.  gev_lineage_seek places a row's cursor on
// the first part with en > x by bisection; gev_lineage_step moves it on while en <= x and labels x by the part it rests on when that
// part's st <= x.  The reductions: gev_lineage_add takes one founder's count into a site record, gev_lineage_merge joins two records of
// disjoint founder sets (sums, the larger top, the lower founder at a tie), so a record may be built in any grouping of the founders.
//
// The first part of this file is plain C++ (gev_dbg_lineage_host and any host program that includes this file alone run the same walk
// and reductions); the kernels behind it need gev_kernels.h (u32, u64).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/geneevolve_amd.h"          // gev_part, gev_lineage_site, GEV_NO_FOUNDER

#if defined(__HIPCC__)
#define GEV_LIN_HD __host__ __device__
#else
#define GEV_LIN_HD
#endif

#ifndef GEV_LINEAGE_TILE
#define GEV_LINEAGE_TILE 16384u                    // founder bins a workgroup histograms at once: 64 KiB of on-chip memory
#endif
#define GEV_LINEAGE_MAX_F 0xfffffffeull            // the most founder haplotypes in all: every fid lies below GEV_NO_FOUNDER
#define GEV_LINEAGE_BAD_POP 1u                     // gev_lineage_check_row: a root population outside [0, n_pop)
#define GEV_LINEAGE_BAD_HAP 2u                     // ... a hap_index at or beyond the founder haplotypes of its root population

// what is wrong with the labels of a row's parts (0: nothing); every part counts, also one that covers nothing
GEV_LIN_HD inline uint32_t gev_lineage_check_row(const gev_part* p, uint32_t n, const uint64_t* n_founder_haps, int n_pop)
{
    uint32_t bad = 0;
    for (uint32_t q = 0; q < n; q++) {
        if (p[q].root_population < 0 || p[q].root_population >= n_pop) bad |= GEV_LINEAGE_BAD_POP;
        else if (p[q].hap_index >= n_founder_haps[p[q].root_population]) bad |= GEV_LINEAGE_BAD_HAP;
    }
    return bad;
}
// the first part of the row with en > x (n: none)
GEV_LIN_HD inline uint32_t gev_lineage_seek(const gev_part* p, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (p[mid].en <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// A row's cursor: the part it rests on is held in `cur` (valid while q < n), so a position that stays inside it reads no memory.
struct GevLineageCursor { uint32_t q; gev_part cur; };
GEV_LIN_HD inline void gev_lineage_place(GevLineageCursor& k, const gev_part* p, uint32_t n, uint64_t x)
{
    k.q = gev_lineage_seek(p, n, x);
    if (k.q < n) k.cur = p[k.q];
}
// the founder id of row p[0..n) at x (checked labels: gev_lineage_check_row); x must not be below the cursor's earlier positions
GEV_LIN_HD inline uint32_t gev_lineage_step(GevLineageCursor& k, const gev_part* p, uint32_t n, uint64_t x, const uint64_t* base)
{
    while (k.q < n && k.cur.en <= x) if (++k.q < n) k.cur = p[k.q];
    if (k.q >= n || k.cur.st > x) return GEV_NO_FOUNDER;
    return (uint32_t)(base[k.cur.root_population] + k.cur.hap_index);
}
GEV_LIN_HD inline gev_lineage_site gev_lineage_empty()
{
    gev_lineage_site s; s.sum_sq = 0; s.n_covered = 0; s.n_lineages = 0; s.top_count = 0; s.top_founder = GEV_NO_FOUNDER;
    return s;
}
// founder f has count k; a caller that adds founders in ascending order may rely on nothing: the lower founder wins a tie in any order
GEV_LIN_HD inline void gev_lineage_add(gev_lineage_site& s, uint32_t f, uint32_t k)
{
    if (!k) return;
    s.sum_sq += (uint64_t)k * k; s.n_covered += k; s.n_lineages++;
    if (k > s.top_count || (k == s.top_count && f < s.top_founder)) { s.top_count = k; s.top_founder = f; }
}
GEV_LIN_HD inline void gev_lineage_merge(gev_lineage_site& s, const gev_lineage_site& o)
{
    s.sum_sq += o.sum_sq; s.n_covered += o.n_covered; s.n_lineages += o.n_lineages;
    if (o.top_count > s.top_count || (o.top_count == s.top_count && o.top_founder < s.top_founder)) { s.top_count = o.top_count; s.top_founder = o.top_founder; }
}
// the host form on lists as gev_download_intervals returns them (off: n_rows + 1 entries), labels checked: base[n_pop + 1] with base[n_pop]
// = F; fid [n_pos][n_rows], counts [n_pos][F], site [n_pos], pop_counts [n_pos][n_pop], each may be NULL.  Position by position with one
// cursor per row; a position's counts are taken in the caller's slice when there is one
inline void gev_lineage_host(const gev_part* parts, const uint64_t* off, size_t n_rows, const uint64_t* pos, size_t n_pos, const uint64_t* base, int n_pop,
                             uint32_t* fid, uint32_t* counts, gev_lineage_site* site, uint32_t* pop_counts)
{
    if (!n_pos) return;
    const size_t F = (size_t)base[n_pop];
    const bool sums = counts || site || pop_counts;
    std::vector<GevLineageCursor> cur(n_rows);
    std::vector<uint32_t> own(sums && !counts ? F : 0);
    for (size_t r = 0; r < n_rows; r++) gev_lineage_place(cur[r], parts + off[r], (uint32_t)(off[r + 1] - off[r]), pos[0]);
    for (size_t p = 0; p < n_pos; p++) {
        uint32_t* cnt = counts ? counts + p * F : own.data();
        if (sums) for (size_t f = 0; f < F; f++) cnt[f] = 0;
        for (size_t r = 0; r < n_rows; r++) {
            const uint32_t id = gev_lineage_step(cur[r], parts + off[r], (uint32_t)(off[r + 1] - off[r]), pos[p], base);
            if (fid) fid[p * n_rows + r] = id;
            if (sums && id != GEV_NO_FOUNDER) cnt[id]++;
        }
        if (site) {
            gev_lineage_site s = gev_lineage_empty();
            for (size_t f = 0; f < F; f++) gev_lineage_add(s, (uint32_t)f, cnt[f]);
            site[p] = s;
        }
        if (pop_counts)
            for (int q = 0; q < n_pop; q++) {
                uint32_t t = 0;
                for (size_t f = (size_t)base[q]; f < (size_t)base[q + 1]; f++) t += cnt[f];
                pop_counts[p * (size_t)n_pop + q] = t;
            }
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// The device, store-and-sum: k_lineage_labels stores every (position, row) label once, k_lineage_sites sums a position's labels per
// founder.  No kernel adds into global memory, so nothing depends on the order workgroups run in.
//
// k_lineage_check: one thread per row of [row0, +n_rows) over all its parts; what gev_lineage_check_row finds is or-ed into *flag (the
// host then hands nothing out).  tab: n_founder_haps[n_pop], then base[n_pop + 1].
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lineage_check(const u32* __restrict__ poff, const gev_part* __restrict__ parts, u64 row0, u32 n_rows,
                                                       const u64* __restrict__ tab, int n_pop, u32* __restrict__ flag)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rows) return;
    const u32 p0 = poff[row0 + r], n = poff[row0 + r + 1] - p0;
    const u32 bad = gev_lineage_check_row(parts + p0, n, (const uint64_t*)tab, n_pop);
    if (bad) atomicOr(flag, bad);
}
// ------------------------------------------------------------------------------------------
// k_lineage_labels: one thread per row, 256 rows a workgroup, consecutive lanes on consecutive rows, over the n_bpos positions of a
// batch (pos: the batch's first).  A lane places its cursor by bisection on the batch's first position, so batches do not depend on each
// other; then all lanes step through the positions together (the position is the same in every lane), each moving its own cursor, and
// store lab[p][row]: one coalesced store of a wave per position.  The part a cursor rests on stays in registers.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lineage_labels(const u32* __restrict__ poff, const gev_part* __restrict__ parts, u64 row0, u32 n_rows,
                                                        const u64* __restrict__ pos, u32 n_bpos, const u64* __restrict__ base, u32* __restrict__ lab)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rows) return;
    const u32 p0 = poff[row0 + r], n = poff[row0 + r + 1] - p0;
    const gev_part* mine = parts + p0;
    GevLineageCursor k;
    gev_lineage_place(k, mine, n, pos[0]);
    for (u32 p = 0; p < n_bpos; p++) lab[(size_t)p * n_rows + r] = gev_lineage_step(k, mine, n, pos[p], (const uint64_t*)base);
}
// the sum of v over the 256 threads of the workgroup, in every thread (w4: 4 words of on-chip memory; two barriers)
__device__ inline u32 lineage_block_sum(u32 v, u32* w4)
{
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    __syncthreads();                                   // (the previous use of w4 has been read)
    if ((threadIdx.x & 63u) == 0) w4[threadIdx.x >> 6] = v;
    __syncthreads();
    return w4[0] + w4[1] + w4[2] + w4[3];
}
// ------------------------------------------------------------------------------------------
// k_lineage_sites: workgroup blockIdx.x = position * n_tiles + tile takes the founders [tile GEV_LINEAGE_TILE, +GEV_LINEAGE_TILE) of one
// position.  It reads the position's label row (n_rows u32; 16-byte loads between a scalar head and tail, the row begins wherever
// p n_rows falls) and counts the ids of its tile in on-chip bins (an id outside the tile, GEV_NO_FOUNDER among them, is passed over).
// Behind a barrier the bins leave as the tile's slice of counts (when wanted), and root population by root population -- their founder
// ranges are contiguous -- the threads reduce them to the tile's site record and per-population sums: a thread's bins ascend, records
// merge by gev_lineage_merge.  The results go to site[blockIdx.x] and pop_counts[blockIdx.x][n_pop]: with one tile these are the call's
// own vectors, with several they are per-tile partials that k_lineage_finish folds.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lineage_sites(const u32* __restrict__ lab, u32 n_rows, const u64* __restrict__ base, int n_pop, u32 F, u32 n_tiles,
                                                       u32* __restrict__ counts, gev_lineage_site* __restrict__ site, u32* __restrict__ pop_counts)
{
    __shared__ __attribute__((aligned(16))) u32 hist[GEV_LINEAGE_TILE];
    __shared__ gev_lineage_site wsite[4];
    __shared__ u32 wsum[4];
    const u32 t = threadIdx.x, p = blockIdx.x / n_tiles, tile = blockIdx.x - p * n_tiles;
    const u32 tile0 = tile * GEV_LINEAGE_TILE, tile_n = F - tile0 < GEV_LINEAGE_TILE ? F - tile0 : GEV_LINEAGE_TILE;
    for (u32 i = t; i < (tile_n + 3u) / 4u; i += 256u) ((uint4*)hist)[i] = make_uint4(0, 0, 0, 0);      // (only the bins in use)
    __syncthreads();
    const u32* row = lab + (size_t)p * n_rows;
    const u32 to16 = (4u - (u32)(((size_t)row >> 2) & 3u)) & 3u, head = to16 < n_rows ? to16 : n_rows, n4 = (n_rows - head) >> 2;
#define GEV_LIN_BIN(id) do { const u32 d_ = (id) - tile0; if (d_ < tile_n) atomicAdd(&hist[d_], 1u); } while (0)
    if (t < head) GEV_LIN_BIN(row[t]);
    const uint4* body = (const uint4*)(row + head);
    for (u32 i = t; i < n4; i += 256u) {
        const uint4 v = body[i];
        GEV_LIN_BIN(v.x); GEV_LIN_BIN(v.y); GEV_LIN_BIN(v.z); GEV_LIN_BIN(v.w);
    }
    if (head + 4u * n4 + t < n_rows) GEV_LIN_BIN(row[head + 4u * n4 + t]);
#undef GEV_LIN_BIN
    __syncthreads();
    if (counts) for (u32 d = t; d < tile_n; d += 256u) counts[(size_t)p * F + tile0 + d] = hist[d];
    gev_lineage_site s = gev_lineage_empty();
    for (int q = 0; q < n_pop; q++) {
        const u64 b0 = base[q], b1 = base[q + 1], lo = b0 > tile0 ? b0 : tile0, hi = b1 < (u64)tile0 + tile_n ? b1 : (u64)tile0 + tile_n;
        u32 sum = 0;
        if (lo < hi) {                                     // (the same in every thread: the barriers inside are reached by all)
            for (u32 d = (u32)(lo - tile0) + t; d < (u32)(hi - tile0); d += 256u) { const u32 k = hist[d]; sum += k; gev_lineage_add(s, tile0 + d, k); }
            sum = lineage_block_sum(sum, wsum);
        }
        if (t == 0) pop_counts[(size_t)blockIdx.x * n_pop + q] = sum;
    }
    for (int d = 32; d; d >>= 1) {
        gev_lineage_site o;
        o.sum_sq = __shfl_down(s.sum_sq, d, 64); o.n_covered = __shfl_down(s.n_covered, d, 64); o.n_lineages = __shfl_down(s.n_lineages, d, 64);
        o.top_count = __shfl_down(s.top_count, d, 64); o.top_founder = __shfl_down(s.top_founder, d, 64);
        gev_lineage_merge(s, o);
    }
    if ((t & 63u) == 0) wsite[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; w++) gev_lineage_merge(s, wsite[w]);
        site[blockIdx.x] = s;
    }
}
// one thread per position of the batch: the n_tiles partial records and per-population sums of the position, folded in tile order
__global__ void __launch_bounds__(256) k_lineage_finish(const gev_lineage_site* __restrict__ psite, const u32* __restrict__ ppop, u32 n_bpos, u32 n_tiles, int n_pop,
                                                        gev_lineage_site* __restrict__ site, u32* __restrict__ pop_counts)
{
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_bpos) return;
    gev_lineage_site s = gev_lineage_empty();
    for (u32 k = 0; k < n_tiles; k++) gev_lineage_merge(s, psite[(size_t)p * n_tiles + k]);
    site[p] = s;
    for (int q = 0; q < n_pop; q++) {
        u32 sum = 0;
        for (u32 k = 0; k < n_tiles; k++) sum += ppop[((size_t)p * n_tiles + k) * n_pop + q];
        pop_counts[(size_t)p * n_pop + q] = sum;
    }
}
#endif
