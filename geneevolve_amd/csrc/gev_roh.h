// gev_roh.h -- runs of homozygosity per individual straight from the haplotype rows: the summary per individual with the cover per SNP
// (gev_roh_summary) and the runs themselves as one ordered list (gev_roh_segments).  The reference has no such output; the truth it is
// held to is a per-SNP walk over the rows gev_download_haps returns (tests/roh_inputs.py, tools/roh_check.cpp).
//
// Definition.  For individual i and the SNP range [snp_begin, snp_begin + n_snps): hom(j) is true when rows 2i and 2i+1 carry the same
// allele at SNP j (mutations applied with the semantics of k_snpmajor_apply_mut / k_snp_apply_mut: !founder at every SNP column whose
// position is in the row's mutation list, idempotent).  A RUN is a maximal set of consecutive SNPs j0..j1 inside the range with hom true
// throughout and, for max_gap_bp != 0, pos[j] - pos[j-1] <= max_gap_bp for every j0 < j <= j1.  SNPs outside the range do not exist for
// the call, so runs are cut at the range's ends: results are NOT additive over SNP ranges.  A run has n = j1 - j0 + 1 SNPs, st = pos[j0]
// and en = pos[j1], both inclusive (PLINK's POS1 and POS2), and en - st base pairs (a one-SNP run has length 0).  It QUALIFIES when
// n >= max(min_snps, 1) and en - st >= min_bp.  SNP columns that share a position are consecutive SNPs with gap 0.  No heterozygous or
// missing call is allowed inside a run.
//
// Word logic.  A row is 64-locus words (locus j = bit j & 63 of word j >> 6).  Per word:
//     h    = ~(a ^ b) & range_mask       the homozygous SNPs of the range (zero outside it, the pad bits beyond L with it)
//     brk  bit j set: a run may not continue from SNP j-1 into j (pos[j] - pos[j-1] > max_gap_bp; all zero for max_gap_bp == 0)
//     start mask = h[j] and not (h[j-1] and not brk[j])        h[j-1] of bit 0: bit 63 of the previous word's h (the carry-in)
//     end mask   = h[j] and not (h[j+1] and not brk[j+1])      bit 63 looks at the next word's first h and brk bits
// a few shifts and ANDs each.  Per end bit the matching start is the highest start bit at or below it in the same word, failing that
// the open start inherited from earlier words (the highest start bit of the nearest earlier word that has one: runs are disjoint, so
// that is the start of the run still open).  Qualification tests n >= min_snps first and loads the two positions only when it holds:
// with a realistic min_snps almost no run gets that far.
//
// The first part of this file is plain C++ (gev_dbg_roh_host and any host program that includes this file alone run the same pieces
// over whole rows: gev_roh_rows_host); the kernels behind it need gev_kernels.h (u32, u64).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/geneevolve_amd.h"          // gev_roh_params, gev_roh_segment

#if defined(__HIPCC__)
#define GEV_ROH_HD __host__ __device__
#else
#define GEV_ROH_HD
#endif

// the bits of word w that lie in [snp_begin, snp_end)
GEV_ROH_HD inline uint64_t gev_roh_range_mask(uint64_t w, uint64_t snp_begin, uint64_t snp_end)
{
    const uint64_t b = w << 6, lo = snp_begin > b ? snp_begin : b, hi = snp_end < b + 64 ? snp_end : b + 64;
    if (lo >= hi) return 0;
    return (hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1ull) << (lo - b);
}
// prev_h: h of SNP j-1 of the previous word (0 or 1)
GEV_ROH_HD inline uint64_t gev_roh_starts(uint64_t h, uint64_t brk, uint64_t prev_h) { return h & ~(((h << 1) | prev_h) & ~brk); }
// next_h, next_brk: the next word's first h and brk bits (0 or 1)
GEV_ROH_HD inline uint64_t gev_roh_ends(uint64_t h, uint64_t brk, uint64_t next_h, uint64_t next_brk)
{
    return h & ~(((h >> 1) | (next_h << 63)) & ~((brk >> 1) | (next_brk << 63)));
}
// the break word w of a chromosome of L positions
GEV_ROH_HD inline uint64_t gev_roh_break_word(const uint64_t* pos, uint64_t L, uint64_t w, uint64_t max_gap_bp)
{
    uint64_t m = 0;
    if (!max_gap_bp) return m;
    const uint64_t b = w << 6, hi = L < b + 64 ? L : b + 64;
    for (uint64_t j = b ? b : 1; j < hi; j++) if (pos[j] - pos[j - 1] > max_gap_bp) m |= 1ull << (j - b);
    return m;
}
GEV_ROH_HD inline unsigned gev_roh_top_bit(uint64_t m) { return 63u - (unsigned)__builtin_clzll(m); }      // m != 0
// the runs that end in a word: emit(j0, n, st, en) for every qualifying one, in SNP order.  base: the SNP of the word's bit 0; open_start:
// the SNP at which the run open at the word's first bit began (read only when there is one)
template <class F>
GEV_ROH_HD inline void gev_roh_word_runs(uint64_t starts, uint64_t ends, uint64_t base, uint64_t open_start, const uint64_t* pos, const gev_roh_params& q, F& emit)
{
    while (ends) {
        const unsigned e = (unsigned)__builtin_ctzll(ends);
        ends &= ends - 1;
        const uint64_t s = starts & ((2ull << e) - 1ull);                      // the start bits at or below e (e = 63: all of them)
        const uint64_t j1 = base + e, j0 = s ? base + gev_roh_top_bit(s) : open_start, n = j1 - j0 + 1;
        if (n < q.min_snps) continue;
        const uint64_t st = pos[j0], en = pos[j1];
        if (en - st < q.min_bp) continue;
        emit(j0, n, st, en);
    }
}
// what the summary keeps of an individual's qualifying runs
struct GevRohSum { uint64_t bp, longest; uint32_t n, snps; };
GEV_ROH_HD inline void gev_roh_add(GevRohSum& s, uint64_t n, uint64_t st, uint64_t en)
{
    s.n++; s.snps += (uint32_t)n; s.bp += en - st;
    if (en - st > s.longest) s.longest = en - st;
}
GEV_ROH_HD inline gev_roh_segment gev_roh_record(uint64_t ind, uint64_t j0, uint64_t n, uint64_t st, uint64_t en)
{
    gev_roh_segment r;
    r.st = st; r.en = en; r.ind = (uint32_t)ind; r.snp_first = (uint32_t)j0; r.n_snps = (uint32_t)n; r.reserved = 0;
    return r;
}
// ---- the reference walk over whole rows in host memory ----
// one individual (rows a, b): emit for every qualifying run of SNPs [snp_begin, +n_snps), in SNP order.  Only the words that hold a SNP
// of the range are read
template <class F>
inline void gev_roh_row_host(const uint64_t* a, const uint64_t* b, const uint64_t* pos, size_t L, size_t snp_begin, size_t n_snps, const gev_roh_params& q, F& emit)
{
    if (!n_snps) return;
    const uint64_t snp_end = snp_begin + n_snps, w0 = snp_begin >> 6, w1 = (snp_end - 1) >> 6;
    uint64_t h = ~(a[w0] ^ b[w0]) & gev_roh_range_mask(w0, snp_begin, snp_end), brk = gev_roh_break_word(pos, L, w0, q.max_gap_bp);
    uint64_t prev_h = 0, open_start = 0;
    for (uint64_t w = w0; w <= w1; w++) {
        const uint64_t next_h = w < w1 ? ~(a[w + 1] ^ b[w + 1]) & gev_roh_range_mask(w + 1, snp_begin, snp_end) : 0;
        const uint64_t next_brk = w < w1 ? gev_roh_break_word(pos, L, w + 1, q.max_gap_bp) : 0;
        const uint64_t starts = gev_roh_starts(h, brk, prev_h), ends = gev_roh_ends(h, brk, next_h & 1u, next_brk & 1u);
        gev_roh_word_runs(starts, ends, w << 6, open_start, pos, q, emit);
        if (starts) open_start = (w << 6) + gev_roh_top_bit(starts);
        prev_h = h >> 63; h = next_h; brk = next_brk;
    }
}
// individuals [ind_begin, +n_ind) of haplotype-major rows (row r = bits + r * row_stride_words).  The four vectors ([n_ind], each may
// be null) are written; diff (null, or n_snps + 1 entries the caller has zeroed) gets +1 at j0 - snp_begin and -1 at j1 + 1 - snp_begin
// of every qualifying run; out (null: nothing is written) gets the records in (ind, snp_first) order.  Returns the number of records
inline uint64_t gev_roh_rows_host(const uint64_t* bits, size_t row_stride_words, const uint64_t* pos, size_t L, size_t snp_begin, size_t n_snps,
                                  size_t ind_begin, size_t n_ind, const gev_roh_params& q,
                                  uint32_t* n_roh, uint64_t* roh_bp, uint32_t* roh_snps, uint64_t* max_bp, uint32_t* diff, gev_roh_segment* out)
{
    uint64_t total = 0;
    for (size_t i = 0; i < n_ind; i++) {
        const uint64_t* a = bits + 2 * (ind_begin + i) * row_stride_words;
        GevRohSum s = {0, 0, 0, 0};
        auto emit = [&](uint64_t j0, uint64_t n, uint64_t st, uint64_t en) {
            gev_roh_add(s, n, st, en);
            if (diff) { diff[j0 - snp_begin]++; diff[j0 + n - snp_begin]--; }
            if (out) out[total + s.n - 1] = gev_roh_record(ind_begin + i, j0, n, st, en);
        };
        gev_roh_row_host(a, a + row_stride_words, pos, L, snp_begin, n_snps, q, emit);
        if (n_roh) n_roh[i] = s.n;
        if (roh_bp) roh_bp[i] = s.bp;
        if (roh_snps) roh_snps[i] = s.snps;
        if (max_bp) max_bp[i] = s.longest;
        total += s.n;
    }
    return total;
}
// cover[j] = the inclusive prefix sum of diff[0 .. j] (n_snps entries; the arrays may be the same)
inline void gev_roh_cover_host(const uint32_t* diff, size_t n_snps, uint32_t* cover)
{
    uint32_t run = 0;
    for (size_t j = 0; j < n_snps; j++) { run += diff[j]; cover[j] = run; }
}
// the capacity rule of gev_roh_segments on the host: *n_total always; out filled if and only if *n_total <= capacity
inline void gev_roh_segments_fit_host(const uint64_t* bits, size_t row_stride_words, const uint64_t* pos, size_t L, size_t snp_begin, size_t n_snps,
                                      size_t ind_begin, size_t n_ind, const gev_roh_params& q, gev_roh_segment* out, size_t capacity, uint64_t* n_total)
{
    *n_total = gev_roh_rows_host(bits, row_stride_words, pos, L, snp_begin, n_snps, ind_begin, n_ind, q, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (*n_total && *n_total <= capacity)
        gev_roh_rows_host(bits, row_stride_words, pos, L, snp_begin, n_snps, ind_begin, n_ind, q, nullptr, nullptr, nullptr, nullptr, nullptr, out);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// The device.  The rows are the staged copy (mutations applied): individual i of a pass = rows 2i, 2i+1 of `chunks` 16-byte chunks.
//
// k_roh_breaks, once per call with max_gap_bp != 0: the break bit plane of the whole chromosome, one thread per word, n_words words
// (an even number that covers L: a lane loads two at a time).
//
// k_roh_scan<MODE>: one wave per individual, four waves a workgroup.  The wave walks the row in tiles of 64 chunks = 128 words = 8192
// SNPs, lane = chunk: one 16-byte load per lane and row, 1 KiB of one row per load instruction (8-byte loads run at 0.54-0.70 of that
// rate), from the chunk that holds snp_begin to the one that holds the last SNP; the next tile's loads are issued before the current
// one is worked on.  A range that begins or ends inside a word, rows longer than a tile and the pad bits beyond L are all the same
// path: the range mask makes h zero outside the range.  Across lanes the carry-in bit (bit 63 of the left neighbour's second word) and
// the next word's first h and brk bits (the right neighbour's first word) come by __shfl_up / __shfl_down; the open start of a lane is
// the wave-wide exclusive prefix maximum of the lanes' last start SNP -- start SNPs grow with the lane, so that maximum is the value of
// the nearest lower lane that has a start at all: one __ballot, one __shfl.  Across tiles the carry-in bit, the open start and the next
// tile's first bits are wave-uniform registers (readfirstlane, the value of lane 63 or of lane 0 of the prefetched tile).
//   ROH_SUMMARY  each lane accumulates count, bp, SNPs and the longest of its qualifying runs; one wave reduction at the end, lane 0
//                stores the four results (entry i of the pass's vectors).  With diff != null a qualifying run adds +1 at diff[j0 -
//                snp_begin] and -1 (mod 2^32) at diff[j1 + 1 - snp_begin] of the zeroed n_snps + 1 entries: integer atomics, the order
//                does not show.  The cover is the inclusive prefix sum of diff (the host runs the tree's scan_u32_on over it).
//   ROH_COUNT    cnt[i] = the individual's qualifying runs.
//   ROH_FILL     cnt is the exclusive scan of those counts.  Per tile the lanes count their qualifying runs, take a wave prefix sum, and
//                write their records from out[cnt[i] + the wave's running base + that prefix] on: an individual's records come out in
//                snp_first order without a sort.  The walk is the count's, so it writes exactly its count.
// Every store is a plain C++ assignment (vector stores).
// ------------------------------------------------------------------------------------------
#define ROH_SUMMARY 0
#define ROH_COUNT 1
#define ROH_FILL 2
#define ROH_TILE_CHUNKS 64u                        // 16-byte chunks of a tile = lanes of a wave
#define ROH_WAVES 4u

__global__ void __launch_bounds__(256) k_roh_breaks(const u64* __restrict__ pos, u64 L, u64 max_gap_bp, u32 n_words, u64* __restrict__ brk)
{
    const u32 w = blockIdx.x * 256u + threadIdx.x;
    if (w < n_words) brk[w] = gev_roh_break_word((const uint64_t*)pos, L, w, max_gap_bp);
}
struct RohDevSum { GevRohSum s; u32* diff; u32 snp_begin;
    __device__ void operator()(uint64_t j0, uint64_t n, uint64_t st, uint64_t en) {
        gev_roh_add(s, n, st, en);
        if (diff) { atomicAdd(diff + (j0 - snp_begin), 1u); atomicAdd(diff + (j0 + n - snp_begin), 0xffffffffu); }
    } };
struct RohDevCount { u32 n; __device__ void operator()(uint64_t, uint64_t, uint64_t, uint64_t) { n++; } };
struct RohDevFill { gev_roh_segment* out; u32 ind; __device__ void operator()(uint64_t j0, uint64_t n, uint64_t st, uint64_t en) { *out++ = gev_roh_record(ind, j0, n, st, en); } };

// n individuals staged from absolute individual ind0 on; the per-individual pointers are the pass's (entry i = individual ind0 + i)
template <int MODE>
__global__ void __launch_bounds__(256) k_roh_scan(const uint4* __restrict__ rows, u32 chunks, u32 n, u32 ind0, const u64* __restrict__ pos,
                                                  const uint4* __restrict__ brk, u32 snp_begin, u32 n_snps, gev_roh_params q,
                                                  u32* __restrict__ n_roh, u64* __restrict__ roh_bp, u32* __restrict__ roh_snps, u64* __restrict__ max_bp, u32* __restrict__ diff,
                                                  u32* __restrict__ cnt, gev_roh_segment* __restrict__ out)
{
    const u32 lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 i = blockIdx.x * ROH_WAVES + wave;
    if (i >= n) return;                                                           // (the whole wave)
    const uint4* ra = rows + (size_t)2 * i * chunks; const uint4* rb = ra + chunks;
    const u64 snp_end = (u64)snp_begin + n_snps;
    const u32 c_first = snp_begin >> 7, c_last = (u32)((snp_end - 1) >> 7), n_tiles = (c_last - c_first) / ROH_TILE_CHUNKS + 1u;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    RohDevSum sum = {{0, 0, 0, 0}, diff, snp_begin};
    RohDevCount count = {0};
    u32 fill_at = MODE == ROH_FILL ? cnt[i] : 0;                                  // where the wave's next record goes
    if (MODE == ROH_FILL && cnt[i + 1] == fill_at) return;
    u32 carry_h = 0, open1 = 0;                                                   // wave-uniform: h of the SNP before the tile; 1 + the last start SNP so far (0: none)
    u32 c = c_first + lane;
    uint4 a = zero, b = zero, k = zero;
    if (c <= c_last) { a = ra[c]; b = rb[c]; if (brk) k = brk[c]; }
    for (u32 t = 0; t < n_tiles; t++) {
        const u32 cn = c + ROH_TILE_CHUNKS;
        uint4 na = zero, nb = zero, nk = zero;
        if (t + 1 < n_tiles && cn <= c_last) { na = ra[cn]; nb = rb[cn]; if (brk) nk = brk[cn]; }
        const u64 w = (u64)2 * c, base0 = w << 6, base1 = base0 + 64;
        const u64 h0 = ~(((u64)a.x | (u64)a.y << 32) ^ ((u64)b.x | (u64)b.y << 32)) & gev_roh_range_mask(w, snp_begin, snp_end);
        const u64 h1 = ~(((u64)a.z | (u64)a.w << 32) ^ ((u64)b.z | (u64)b.w << 32)) & gev_roh_range_mask(w + 1, snp_begin, snp_end);
        const u64 k0 = (u64)k.x | (u64)k.y << 32, k1 = (u64)k.z | (u64)k.w << 32;
        // the first h and brk bits behind the tile: lane 0 of the prefetched one (zero behind the last tile: its words lie beyond the range)
        const u32 tile_next_h = __builtin_amdgcn_readfirstlane((u32)(~(na.x ^ nb.x) & (u32)gev_roh_range_mask((u64)2 * cn, snp_begin, snp_end) & 1u));
        const u32 tile_next_k = __builtin_amdgcn_readfirstlane(nk.x & 1u);
        u32 prev_h = __shfl_up((u32)(h1 >> 63), 1), next_h = __shfl_down((u32)h0 & 1u, 1), next_k = __shfl_down((u32)k0 & 1u, 1);
        if (lane == 0) prev_h = carry_h;
        if (lane == 63) { next_h = tile_next_h; next_k = tile_next_k; }
        const u64 starts0 = gev_roh_starts(h0, k0, prev_h), starts1 = gev_roh_starts(h1, k1, h0 >> 63);
        const u64 ends0 = gev_roh_ends(h0, k0, h1 & 1u, k1 & 1u), ends1 = gev_roh_ends(h1, k1, next_h, next_k);
        // 1 + the lane's last start SNP (0: none), and the open start of its first word: the nearest lower lane's that has one, else the tiles' before
        const u32 last1 = starts1 ? (u32)(base1 + gev_roh_top_bit(starts1)) + 1u : starts0 ? (u32)(base0 + gev_roh_top_bit(starts0)) + 1u : 0u;
        const u64 have = __ballot(last1 != 0), below = have & ((1ull << lane) - 1ull);
        const u32 from = __shfl(last1, below ? (int)gev_roh_top_bit(below) : 0);
        // (0 - 1: no run is open.  No end bit asks then: an end bit without a start bit at or below it in its word has h set from bit 0
        // of the word up to it with no break and, not being a start itself, a set carry-in, so a run that began in the range is open)
        const u32 open0 = (below ? from : open1) - 1u;
        const u32 open_1 = starts0 ? (u32)(base0 + gev_roh_top_bit(starts0)) : open0;
        if (MODE == ROH_SUMMARY) {
            gev_roh_word_runs(starts0, ends0, base0, open0, (const uint64_t*)pos, q, sum);
            gev_roh_word_runs(starts1, ends1, base1, open_1, (const uint64_t*)pos, q, sum);
        } else if (MODE == ROH_COUNT) {
            gev_roh_word_runs(starts0, ends0, base0, open0, (const uint64_t*)pos, q, count);
            gev_roh_word_runs(starts1, ends1, base1, open_1, (const uint64_t*)pos, q, count);
        } else if (__ballot((ends0 | ends1) != 0)) {
            RohDevCount mine = {0};
            gev_roh_word_runs(starts0, ends0, base0, open0, (const uint64_t*)pos, q, mine);
            gev_roh_word_runs(starts1, ends1, base1, open_1, (const uint64_t*)pos, q, mine);
            if (__ballot(mine.n != 0)) {
                u32 inc = mine.n;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const u32 o = __shfl_up(inc, d); if (lane >= (u32)d) inc += o; }
                if (mine.n) {
                    RohDevFill f = {out + fill_at + (inc - mine.n), ind0 + i};
                    gev_roh_word_runs(starts0, ends0, base0, open0, (const uint64_t*)pos, q, f);
                    gev_roh_word_runs(starts1, ends1, base1, open_1, (const uint64_t*)pos, q, f);
                }
                fill_at += __shfl(inc, 63);
            }
        }
        if (have) open1 = __builtin_amdgcn_readfirstlane(__shfl(last1, (int)gev_roh_top_bit(have)));
        carry_h = __builtin_amdgcn_readfirstlane(__shfl((u32)(h1 >> 63), 63));
        a = na; b = nb; k = nk; c = cn;
    }
    if (MODE == ROH_SUMMARY) {
        GevRohSum s = sum.s;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            s.n += __shfl_down(s.n, d); s.snps += __shfl_down(s.snps, d); s.bp += __shfl_down(s.bp, d);
            const u64 o = __shfl_down(s.longest, d);
            if (o > s.longest) s.longest = o;
        }
        if (lane == 0) { n_roh[i] = s.n; roh_bp[i] = s.bp; roh_snps[i] = s.snps; max_bp[i] = s.longest; }
    }
    if (MODE == ROH_COUNT) {
        u32 s = count.n;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
        if (lane == 0) cnt[i] = s;
    }
}
#endif
