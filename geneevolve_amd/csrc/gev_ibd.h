// gev_ibd.h -- identity by descent per pair of haplotype rows from the ancestry interval lists: three summaries per pair
// (gev_ibd_sharing) and the segments themselves as one ordered list (gev_ibd_segments); and the base pairs of a row by root
// population (gev_ancestry_bp).  The reference has no such output; the truth it is held to is a per-position raster of the lists
// gev_download_intervals returns (tests/ibd_inputs.py, tests/ibd_segments_inputs.py, tools/ibd_check.cpp, tools/ibd_segments_check.cpp).
//
// A row's list is what the library keeps for it: gev_part records in position order, half-open [st, en), no two overlapping (gaps,
// rows without parts and parts with st >= en, which cover nothing, are allowed).  f_r(x) = (root_population, hap_index) of the part
// of row r that covers x.  The IBD set of rows r, s is {x : f_r(x) and f_s(x) defined and equal}; its segments are its maximal
// intervals.  Over the segments of length >= min_bp:  shared_bp = their summed length (u64), n_seg = their number (u32), max_seg =
// the longest (u64, 0 without one).  Plain 64-bit integers, labels compared whole: exact and the same on every run.
//
// The walk (gev_ibd_walk, one source for the device and the host): two cursors; the overlap [max(st), min(en)) of the two current
// parts, when it is not empty and the labels agree, extends the open run if it begins where the run ended and otherwise closes the
// run and opens another; the list whose part ends first moves on (both when they end together); a closed run of length >= min_bp is
// added to the three results.  The overlaps come in position order and are disjoint, so a run is broken exactly where a position is
// not shared: a segment runs on across a common change of founder and across adjacent parts of one row with the same label.
//
// The first part of this file is plain C++ (gev_dbg_ibd_host and any host program that includes this file alone run the same walk);
// the kernels behind it need gev_kernels.h (u32, u64).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/geneevolve_amd.h"          // gev_part

#if defined(__HIPCC__)
#define GEV_IBD_HD __host__ __device__
#else
#define GEV_IBD_HD
#endif

#define GEV_IBD_TILE 16u                           // rows a side of a workgroup's tile: 256 pairs, one per lane

struct GevIbdRun { uint64_t shared, longest; uint32_t n; };

GEV_IBD_HD inline void gev_ibd_close(GevIbdRun& r, uint64_t len, uint64_t min_bp)
{
    if (len < min_bp) return;
    r.shared += len; r.n++;
    if (len > r.longest) r.longest = len;
}
// the pair's results from the two lists (na, nb parts; either may be 0)
GEV_IBD_HD inline GevIbdRun gev_ibd_walk(const gev_part* pa, uint32_t na, const gev_part* pb, uint32_t nb, uint64_t min_bp)
{
    GevIbdRun r = {0, 0, 0};
    if (!na || !nb) return r;
    uint32_t i = 0, j = 0;
    gev_part A = pa[0], B = pb[0];
    uint64_t run_st = 0, run_en = 0;
    bool open = false;
    for (;;) {
        const uint64_t lo = A.st > B.st ? A.st : B.st, hi = A.en < B.en ? A.en : B.en;
        if (lo < hi && A.hap_index == B.hap_index && A.root_population == B.root_population) {
            if (open && lo == run_en) run_en = hi;
            else {
                if (open) gev_ibd_close(r, run_en - run_st, min_bp);
                run_st = lo; run_en = hi; open = true;
            }
        }
        const bool adv_a = A.en <= B.en, adv_b = B.en <= A.en;
        if (adv_a) { if (++i == na) break; A = pa[i]; }
        if (adv_b) { if (++j == nb) break; B = pb[j]; }
    }
    if (open) gev_ibd_close(r, run_en - run_st, min_bp);
    return r;
}
// the host form on lists as gev_download_intervals returns them (off_*: n_* + 1 entries): row-major [n_a][n_b], each output may be NULL
inline void gev_ibd_host(const gev_part* parts_a, const uint64_t* off_a, size_t n_a, const gev_part* parts_b, const uint64_t* off_b, size_t n_b,
                         uint64_t min_bp, uint64_t* shared_bp, uint32_t* n_seg, uint64_t* max_seg)
{
    for (size_t a = 0; a < n_a; a++)
        for (size_t b = 0; b < n_b; b++) {
            const uint32_t la = (uint32_t)(off_a[a + 1] - off_a[a]), lb = (uint32_t)(off_b[b + 1] - off_b[b]);
            const GevIbdRun r = gev_ibd_walk(la ? parts_a + off_a[a] : nullptr, la, lb ? parts_b + off_b[b] : nullptr, lb, min_bp);
            if (shared_bp) shared_bp[a * n_b + b] = r.shared;
            if (n_seg) n_seg[a * n_b + b] = r.n;
            if (max_seg) max_seg[a * n_b + b] = r.longest;
        }
}
// ---- the segments themselves (gev_ibd_segments) ----
// The same walk with an emit point in place of the three sums: emit(st, en) is called for every closed run of length >= min_bp, in
// position order.  It stands beside gev_ibd_walk, which k_ibd_tiles keeps as it was measured; a count, a fill
// and the host form are this one function under three functors.
template <class F>
GEV_IBD_HD inline void gev_ibd_walk_emit(const gev_part* pa, uint32_t na, const gev_part* pb, uint32_t nb, uint64_t min_bp, F& emit)
{
    if (!na || !nb) return;
    uint32_t i = 0, j = 0;
    gev_part A = pa[0], B = pb[0];
    uint64_t run_st = 0, run_en = 0;
    bool open = false;
    for (;;) {
        const uint64_t lo = A.st > B.st ? A.st : B.st, hi = A.en < B.en ? A.en : B.en;
        if (lo < hi && A.hap_index == B.hap_index && A.root_population == B.root_population) {
            if (open && lo == run_en) run_en = hi;
            else {
                if (open && run_en - run_st >= min_bp) emit(run_st, run_en);
                run_st = lo; run_en = hi; open = true;
            }
        }
        const bool adv_a = A.en <= B.en, adv_b = B.en <= A.en;
        if (adv_a) { if (++i == na) break; A = pa[i]; }
        if (adv_b) { if (++j == nb) break; B = pb[j]; }
    }
    if (open && run_en - run_st >= min_bp) emit(run_st, run_en);
}
struct GevIbdCount { uint32_t n; GEV_IBD_HD void operator()(uint64_t, uint64_t) { n++; } };
// writes the records of one pair one behind the other: a plain assignment of the 8-byte-aligned record (vector stores on the device)
struct GevIbdFill {
    gev_ibd_segment* out; uint32_t row_a, row_b;
    GEV_IBD_HD void operator()(uint64_t st, uint64_t en) { gev_ibd_segment s; s.st = st; s.en = en; s.row_a = row_a; s.row_b = row_b; *out++ = s; }
};
// the host form: the records of all pairs in (row_a, row_b, st) order, rows numbered by their index in off_*; upper: only pairs with
// a < b.  out null: nothing is written.  Returns the number of records; a caller fills a buffer it has sized by a first, counting call
inline uint64_t gev_ibd_segments_host(const gev_part* parts_a, const uint64_t* off_a, size_t n_a, const gev_part* parts_b, const uint64_t* off_b, size_t n_b,
                                      uint64_t min_bp, bool upper, gev_ibd_segment* out)
{
    uint64_t total = 0;
    for (size_t a = 0; a < n_a; a++)
        for (size_t b = upper ? a + 1 : 0; b < n_b; b++) {
            const uint32_t la = (uint32_t)(off_a[a + 1] - off_a[a]), lb = (uint32_t)(off_b[b + 1] - off_b[b]);
            const gev_part* pa = la ? parts_a + off_a[a] : nullptr; const gev_part* pb = lb ? parts_b + off_b[b] : nullptr;
            if (out) {
                GevIbdFill f = {out + total, (uint32_t)a, (uint32_t)b};
                gev_ibd_walk_emit(pa, la, pb, lb, min_bp, f);
                total += (uint64_t)(f.out - (out + total));
            } else {
                GevIbdCount k = {0};
                gev_ibd_walk_emit(pa, la, pb, lb, min_bp, k);
                total += k.n;
            }
        }
    return total;
}
// the capacity rule of gev_ibd_segments on the host: *n_total always; out filled if and only if *n_total <= capacity
inline void gev_ibd_segments_fit_host(const gev_part* parts_a, const uint64_t* off_a, size_t n_a, const gev_part* parts_b, const uint64_t* off_b, size_t n_b,
                                      uint64_t min_bp, bool upper, gev_ibd_segment* out, size_t capacity, uint64_t* n_total)
{
    *n_total = gev_ibd_segments_host(parts_a, off_a, n_a, parts_b, off_b, n_b, min_bp, upper, nullptr);
    if (*n_total && *n_total <= capacity) gev_ibd_segments_host(parts_a, off_a, n_a, parts_b, off_b, n_b, min_bp, upper, out);
}
// base pairs of one row by root population into bp[n_pop] (zeroed here); false, with bp left as it is, when a part's root population lies
// outside [0, n_pop).  A part with st >= en covers nothing
GEV_IBD_HD inline bool gev_ancestry_row(const gev_part* p, uint32_t n, int n_pop, uint64_t* bp)
{
    for (uint32_t q = 0; q < n; q++) if (p[q].root_population < 0 || p[q].root_population >= n_pop) return false;
    for (int k = 0; k < n_pop; k++) bp[k] = 0;
    for (uint32_t q = 0; q < n; q++) if (p[q].en > p[q].st) bp[p[q].root_population] += p[q].en - p[q].st;
    return true;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// The device.  k_ibd_tiles: a workgroup of 256 threads takes a tile of 16 rows of side A x 16 rows of side B of a sub-block of the
// pair matrix (blockIdx.y, blockIdx.x), one pair per lane; wave w takes the 8 x 8 block of pairs at (8 (w >> 1), 8 (w & 1)), A row
// lane >> 3, B row lane & 7, so a wave's loads touch 8 + 8 lists, not 64.  The lanes walk the lists where they lie: read-only loads,
// a tile's 32 lists stay in the caches.  Nothing bounds a row's length.  The kernel uses no on-chip memory: what it is worth is waves
// in flight, since every step of a walk waits for the load of the next part (a copy of the tile's lists in
// on-chip memory was measured and lost to this form as soon as its reservation cost a wave).  An output that is null is not stored;
// every store is a vector store.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ibd_tiles(const u32* __restrict__ poff_a, const gev_part* __restrict__ parts_a, u64 row_a, u32 n_a,
                                                   const u32* __restrict__ poff_b, const gev_part* __restrict__ parts_b, u64 row_b, u32 n_b,
                                                   u64 min_bp, u64* __restrict__ shared_bp, u32* __restrict__ n_seg, u64* __restrict__ max_seg)
{
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const u32 ia = blockIdx.y * GEV_IBD_TILE + 8u * (wave >> 1) + (lane >> 3), ib = blockIdx.x * GEV_IBD_TILE + 8u * (wave & 1u) + (lane & 7u);
    if (ia >= n_a || ib >= n_b) return;
    const u32* oa = poff_a + row_a + ia; const u32* ob = poff_b + row_b + ib;
    const u32 pa0 = oa[0], na = oa[1] - pa0, pb0 = ob[0], nb = ob[1] - pb0;
    const GevIbdRun r = gev_ibd_walk(parts_a + pa0, na, parts_b + pb0, nb, min_bp);
    const size_t o = (size_t)ia * n_b + ib;
    if (shared_bp) shared_bp[o] = r.shared;
    if (n_seg) n_seg[o] = r.n;
    if (max_seg) max_seg[o] = r.longest;
}
// ------------------------------------------------------------------------------------------
// k_ibd_segments: the count and the fill of gev_ibd_segments over one strip of n_a whole A rows against n_b B rows (row_a, row_b: the
// absolute rows of the strip's first pair, which are also what the records name).  The geometry is k_ibd_tiles': 256 pairs a workgroup,
// one per lane, 64 a wave in a block of rows so that a wave's loads touch few lists; no on-chip memory.  A tile is 2^ta_log2 A rows x
// 2^(8 - ta_log2) B rows, a wave's block min(2^ta_log2, 8) A rows x the B rows that make 64: ta_log2 = 4 is the 16 x 16 tile with 8 x 8
// wave blocks, and a strip of fewer than 16 rows takes the smallest power of two that holds it (8 x 32, 4 x 64, 2 x 128, 1 x 256), so
// that at least half of a tile's A rows exist.  Tiles are numbered B-fastest in blockIdx.x (tiles_b a tile row).
//   FILL = false: cnt[ia][ib] = the pair's records (u32 [n_a][n_b]).  upper: lanes with row_a >= row_b store nothing and tiles wholly
//                 on or below the diagonal return at once, so the host zeroes cnt first.
//   FILL = true:  cnt is the exclusive scan of those counts (n_a n_b + 1 entries); a pair with records walks again and writes them from
//                 out[cnt[pair]] on, a pair without returns.  The walk is the count's, so it writes exactly its count.
// ------------------------------------------------------------------------------------------
template <bool FILL>
__global__ void __launch_bounds__(256) k_ibd_segments(const u32* __restrict__ poff_a, const gev_part* __restrict__ parts_a, u64 row_a, u32 n_a,
                                                      const u32* __restrict__ poff_b, const gev_part* __restrict__ parts_b, u64 row_b, u32 n_b,
                                                      u64 min_bp, u32 upper, u32 ta_log2, u32 tiles_b, u32* __restrict__ cnt, gev_ibd_segment* __restrict__ out)
{
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const u32 tb_log2 = 8u - ta_log2, wa_log2 = ta_log2 < 3u ? ta_log2 : 3u, wb_log2 = 6u - wa_log2, waves_a_log2 = ta_log2 - wa_log2;    // (waves_a_log2: 1 for the 16-row tile, else 0)
    const u32 tile_a = blockIdx.x / tiles_b, tile_b = blockIdx.x - tile_a * tiles_b;
    const u64 a0 = (u64)tile_a << ta_log2, b0 = (u64)tile_b << tb_log2;
    if (upper && row_b + b0 + (1u << tb_log2) - 1u <= row_a + a0) return;                     // the tile's last B row is no later than its first A row
    const u64 ia = a0 + ((wave >> (2u - waves_a_log2)) << wa_log2) + (lane >> wb_log2);
    const u64 ib = b0 + ((wave & ((4u >> waves_a_log2) - 1u)) << wb_log2) + (lane & ((1u << wb_log2) - 1u));
    if (ia >= n_a || ib >= n_b) return;
    const u64 ra = row_a + ia, rb = row_b + ib;
    if (upper && ra >= rb) return;
    const size_t o = (size_t)ia * n_b + ib;
    const u32* oa = poff_a + ra; const u32* ob = poff_b + rb;
    const u32 pa0 = oa[0], na = oa[1] - pa0, pb0 = ob[0], nb = ob[1] - pb0;
    if (FILL) {
        const u32 at = cnt[o];
        if (cnt[o + 1] == at) return;
        GevIbdFill f = {out + at, (u32)ra, (u32)rb};
        gev_ibd_walk_emit(parts_a + pa0, na, parts_b + pb0, nb, min_bp, f);
    } else {
        GevIbdCount k = {0};
        gev_ibd_walk_emit(parts_a + pa0, na, parts_b + pb0, nb, min_bp, k);
        cnt[o] = k.n;
    }
}
// one thread per row of [row0, +n_rows): bp[r][n_pop] and n_parts[r]; a root population outside [0, n_pop) raises *flag (the host then
// hands nothing out)
__global__ void __launch_bounds__(256) k_ancestry_bp(const u32* __restrict__ poff, const gev_part* __restrict__ parts, u64 row0, u32 n_rows, int n_pop,
                                                     u64* __restrict__ bp, u32* __restrict__ n_parts, u32* __restrict__ flag)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rows) return;
    const u32 p0 = poff[row0 + r], n = poff[row0 + r + 1] - p0;
    n_parts[r] = n;
    if (!gev_ancestry_row(parts + p0, n, n_pop, (uint64_t*)bp + (size_t)r * n_pop)) atomicOr(flag, 1u);
}
#endif
