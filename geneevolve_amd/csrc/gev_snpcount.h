// gev_snpcount.h -- genotype counts per SNP straight from the resident haplotype-major rows (gev_snp_genotype_counts): for every SNP of a
// range, over the individuals of a range, how many are heterozygous and how many carry allele 1 twice.  The reference has no such
// output; the truth it is held to is a column count over the rows gev_download_haps returns.
//
// A column count over bit rows is a positional popcount.  Rows 2i and 2i+1 are individual i's haplotypes, so per individual
//     x = a ^ b   (heterozygous)        y = a & b   (allele 1 on both)
// and each of the two is added into a VERTICAL counter: level k of a counter is one machine word that holds bit k of the running
// count of every locus of the word.  Adding a word is a ripple of half adders over the levels,
//     carry = c[k] & v;  c[k] ^= v;  v = carry
// two operations per level, whatever the number of loci in the word.  GEV_SNPC_K levels count to GEV_SNPC_F = 2^K - 1, so after F
// individuals -- the only moment the top level could overflow -- the levels are expanded to one integer per locus, handed to a sink
// and cleared.  The sink gets the two counts of a locus packed in one word (heterozygous in the low half, homozygous in the high
// one): both stay below 2^16 for as long as a sink adds fewer than 65 536 individuals into one word.
//
// K = 6: per individual and word 12 operations per counter for the adds, and an expansion of 2 * K operations per locus every 63
// individuals.  For the device's 128-locus words that is 104 + 8 operations per individual for the adds and 3072 / 63 = 49 for the
// expansions; K = 5 gives 88 + 83, K = 7 120 + 28, K = 8 136 + 16 -- the sum is flat from 6 to 8 and 6 keeps the fewest registers
// (2 * K * 4 for the levels).
//
// The first part of this file is plain C++ (host and device from one source: gev_dbg_snp_counts_host runs it on rows in host
// memory, and so does any host program that includes this file alone); the kernels behind it need gev_kernels.h (RowMap).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GEV_SNPC_HD __host__ __device__
#else
#define GEV_SNPC_HD
#endif

#define GEV_SNPC_K 6                              // levels of a vertical counter
#define GEV_SNPC_F ((1u << GEV_SNPC_K) - 1u)     // individuals a counter takes before it must be expanded
#define GEV_SNPC_BATCH 4                          // individuals whose rows are loaded before any of them is added (loads in flight)

// a machine word of loci: COMPS components of BITS bits, locus comp * BITS + b = bit b of component comp
template <class W> struct GevSnpcWord;
template <> struct GevSnpcWord<uint64_t> {
    static constexpr unsigned COMPS = 1, BITS = 64;
    static GEV_SNPC_HD uint32_t bit(uint64_t w, unsigned, unsigned b) { return (uint32_t)(w >> b) & 1u; }
};

template <class W> struct GevSnpcCounter {
    W het[GEV_SNPC_K], hom[GEV_SNPC_K];           // level k = bit k of the two running counts of every locus of the word
    uint32_t pending;                             // individuals added since the levels were last empty (at most GEV_SNPC_F)
};
template <class W> GEV_SNPC_HD inline void gev_snpc_clear(GevSnpcCounter<W>& c)
{
#pragma unroll
    for (int k = 0; k < GEV_SNPC_K; k++) { c.het[k] = W(0); c.hom[k] = W(0); }
    c.pending = 0;
}
// one individual: haplotype words a and b
template <class W> GEV_SNPC_HD inline void gev_snpc_add(GevSnpcCounter<W>& c, W a, W b)
{
    W x = a ^ b, y = a & b;
#pragma unroll
    for (int k = 0; k < GEV_SNPC_K; k++) { const W carry = c.het[k] & x; c.het[k] ^= x; x = carry; }
#pragma unroll
    for (int k = 0; k < GEV_SNPC_K; k++) { const W carry = c.hom[k] & y; c.hom[k] ^= y; y = carry; }
    c.pending++;
}
// the levels as integers: sink(locus of the word, heterozygous | homozygous << 16) for every locus with a count; the counter is empty after
template <class W, class Sink> GEV_SNPC_HD inline void gev_snpc_expand(GevSnpcCounter<W>& c, Sink& sink)
{
    typedef GevSnpcWord<W> T;
    for (unsigned b = 0; b < T::BITS; b++) {
#pragma unroll
        for (unsigned comp = 0; comp < T::COMPS; comp++) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < GEV_SNPC_K; k++) v |= (T::bit(c.het[k], comp, b) << k) | (T::bit(c.hom[k], comp, b) << (16 + k));
            if (v) sink(comp * T::BITS + b, v);
        }
    }
    gev_snpc_clear(c);
}
// n_ind individuals through one counter: locate(i) says where the two haplotype words of individual i lie (on the device: looks the
// rows' units up), fetch(where, a, b) loads them; a batch is located, then fetched, then added, so that its loads are in flight
// together.  The counter is expanded into the sink whenever it is full and once at the end
template <class W, class Locate, class Fetch, class Sink> GEV_SNPC_HD inline void gev_snpc_run(size_t n_ind, Locate locate, Fetch fetch, Sink sink)
{
    typedef decltype(locate((size_t)0)) Where;
    GevSnpcCounter<W> c;
    gev_snpc_clear(c);
    size_t i = 0;
    for (; i + GEV_SNPC_BATCH <= n_ind; i += GEV_SNPC_BATCH) {
        Where at[GEV_SNPC_BATCH];
        W a[GEV_SNPC_BATCH], b[GEV_SNPC_BATCH];
#pragma unroll
        for (int u = 0; u < GEV_SNPC_BATCH; u++) at[u] = locate(i + u);
#pragma unroll
        for (int u = 0; u < GEV_SNPC_BATCH; u++) fetch(at[u], a[u], b[u]);
#pragma unroll
        for (int u = 0; u < GEV_SNPC_BATCH; u++) {
            gev_snpc_add(c, a[u], b[u]);
            if (c.pending == GEV_SNPC_F) gev_snpc_expand(c, sink);
        }
    }
    for (; i < n_ind; i++) {
        W a, b;
        fetch(locate(i), a, b);
        gev_snpc_add(c, a, b);
        if (c.pending == GEV_SNPC_F) gev_snpc_expand(c, sink);
    }
    if (c.pending) gev_snpc_expand(c, sink);
}
// haplotype-major rows in host memory (row r = bits + r * row_stride_words, locus j = bit j & 63 of word j >> 6, rows 2i and 2i+1 =
// individual i): the counts of SNPs [snp_begin, +n_snps) over individuals [0, n_ind).  Only the words that hold a SNP of the range
// are read; what they hold outside the range is counted with the rest and dropped when the counter is expanded.
inline void gev_snpc_count_rows_host(const uint64_t* bits, size_t row_stride_words, size_t n_ind, size_t snp_begin, size_t n_snps,
                                     uint32_t* n_het, uint32_t* n_hom_alt)
{
    for (size_t j = 0; j < n_snps; j++) n_het[j] = n_hom_alt[j] = 0;
    if (!n_snps || !n_ind) return;
    const size_t snp_end = snp_begin + n_snps;
    for (size_t w = snp_begin >> 6; w <= (snp_end - 1) >> 6; w++)
        gev_snpc_run<uint64_t>(n_ind,
            [&](size_t i) { return bits + 2 * i * row_stride_words + w; },
            [&](const uint64_t* at, uint64_t& a, uint64_t& b) { a = at[0]; b = at[row_stride_words]; },
            [&](unsigned locus, uint32_t v) {
                const size_t g = (w << 6) + locus;
                if (g >= snp_begin && g < snp_end) { n_het[g - snp_begin] += v & 0xffffu; n_hom_alt[g - snp_begin] += v >> 16; }
            });
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------
// The device: two kernels that add into the same two uint32 vectors (zeroed by the caller; integer adds commute, so neither their
// order nor the order of the blocks shows in the result).
//
// 1. k_snp_counts, the plane pass.  The plane holds FOUNDER alleles.  A thread owns one 16-byte chunk column (128 loci, a v4u word)
// and walks a run of individuals down it; the 64 lanes of a wave own the 64 chunks of one 1 KiB-aligned piece of the row, so every
// load instruction of a wave reads 1 KiB of one row -- in place through the rows' unit table, no staging copy, no transpose.  With
// segments of 1 KiB or more (the default is 2 KiB) the piece lies in ONE unit: SAME_UNIT looks it up once per wave (a scalar load,
// scalar address arithmetic); with smaller segments every lane looks its own unit up.  The grid is cut over the 64-chunk pieces that
// hold a SNP of the range (x) and blocks of individuals (y); the four waves of a workgroup take a quarter of the block's individuals
// each and expand into ONE partial in LDS (128 loci x 64 columns of packed counts, padded to a pitch of 65 words so that both the
// waves' adds, lane = column, and the final sweep, thread = locus, are free of bank conflicts).  At the end the workgroup adds its
// partial to the global vectors, and only there the SNP range is applied: chunks that hold no SNP of the range are never read, bits
// of the first and last chunk outside it (the pad bits beyond L among them) are counted in registers and dropped here.
// ind_per_block <= SNPC_MAX_IND keeps both halves of a packed count below 2^16.
//
// 2. k_snp_counts_apply_mut, the mutation overlay, with the semantics of k_snpmajor_apply_mut: a haplotype's value at every SNP
// column whose position is in its mutation list is !founder -- idempotent, so a position repeated in a list counts once, and every
// column that shares the position is hit.  One thread per individual merges the two (ascending) lists; per distinct position and
// column it reads the two founder bits, derives the genotype before and after the flips and corrects the two counts by +-1.  Sparse:
// the cost follows the number of mutations, not L.
// ------------------------------------------------------------------------------------------
template <> struct GevSnpcWord<v4u> {
    static constexpr unsigned COMPS = 4, BITS = 32;
    static __device__ __forceinline__ uint32_t bit(v4u w, unsigned comp, unsigned b) { return (w[comp] >> b) & 1u; }
};
#define SNPC_COLS 64u                             // chunk columns of a workgroup = lanes of a wave
#define SNPC_WAVES 4u
#define SNPC_LOCI 128u                            // loci of a chunk
#define SNPC_PITCH (SNPC_COLS + 1u)
#define SNPC_MAX_IND 32768u                       // individuals of a workgroup (packed 16-bit halves in its partial)
static_assert(GEV_SNPC_F < 65536u && SNPC_MAX_IND < 65536u, "a packed count keeps each half in 16 bits");

struct SnpcWhere { const uint4 *a, *b; };       // the chunk of an individual's two haplotype rows
// individuals [ind_begin, ind_begin + n_ind), chunks [q_first, q_first + n_q) of their rows; blockIdx.x = 64-chunk piece of the row
// counted from the piece that holds q_first, blockIdx.y = block of ind_per_block individuals.  n_het / n_hom: [n_snps], entry j = SNP
// snp_begin + j.  SAME_UNIT: rm.seg_shift >= 6
template <bool SAME_UNIT>
__global__ void __launch_bounds__(256) k_snp_counts(RowMap rm, size_t ind_begin, size_t n_ind, u32 ind_per_block, u32 q_first, u32 n_q,
                                                    u32 snp_begin, u32 n_snps, u32* __restrict__ n_het, u32* __restrict__ n_hom)
{
    __shared__ u32 part[SNPC_LOCI * SNPC_PITCH];
    for (u32 t = threadIdx.x; t < SNPC_LOCI * SNPC_PITCH; t += SNPC_WAVES * 64u) part[t] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 piece0 = (q_first / SNPC_COLS + blockIdx.x) * SNPC_COLS;                  // first chunk of the workgroup's piece
    const size_t b0 = (size_t)blockIdx.y * ind_per_block, b1 = b0 + ind_per_block < n_ind ? b0 + ind_per_block : n_ind;
    const size_t per = (b1 - b0 + SNPC_WAVES - 1) / SNPC_WAVES;
    const size_t w0 = b0 + wave * per < b1 ? b0 + wave * per : b1, w1 = w0 + per < b1 ? w0 + per : b1;
    const u32 q = piece0 + lane;
    if (q >= q_first && q - q_first < n_q && w0 < w1) {
        const size_t first = ind_begin + w0;
        const u32 seg = SAME_UNIT ? piece0 >> rm.seg_shift : q >> rm.seg_shift, within = q & ((1u << rm.seg_shift) - 1u);
        gev_snpc_run<v4u>(w1 - w0,
            [&](size_t i) {
                const size_t at = 2 * (first + i) * rm.nseg + seg;                      // (SAME_UNIT: the same for the whole wave)
                const u32 ua = rm.phys[at], ub = rm.phys[at + rm.nseg];
                return SnpcWhere{(const uint4*)(rm.pool + ((size_t)ua << (rm.seg_shift + 4))) + within, (const uint4*)(rm.pool + ((size_t)ub << (rm.seg_shift + 4))) + within};
            },
            [&](const SnpcWhere& at, v4u& a, v4u& b) {
                const uint4 ra = *at.a, rb = *at.b;
                a = v4u{ra.x, ra.y, ra.z, ra.w}; b = v4u{rb.x, rb.y, rb.z, rb.w};
            },
            [&](unsigned locus, u32 v) { atomicAdd(&part[locus * SNPC_PITCH + lane], v); });
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < SNPC_LOCI * SNPC_COLS; t += SNPC_WAVES * 64u) {
        const u32 col = t / SNPC_LOCI, locus = t % SNPC_LOCI;
        const u64 g = (u64)(piece0 + col) * SNPC_LOCI + locus;
        if (g < snp_begin || g - snp_begin >= n_snps) continue;
        const u32 v = part[locus * SNPC_PITCH + col];
        if (v & 0xffffu) atomicAdd(n_het + (g - snp_begin), v & 0xffffu);
        if (v >> 16) atomicAdd(n_hom + (g - snp_begin), v >> 16);
    }
}
// m_off / m_pos: the CSR mutation lists of the current generation (ascending per row); pos: the chromosome's SNP positions
__global__ void __launch_bounds__(256) k_snp_counts_apply_mut(RowMap rm, size_t ind_begin, size_t n_ind, const u32* __restrict__ m_off, const u64* __restrict__ m_pos,
                                                              const u64* __restrict__ pos, u32 snp_begin, u32 n_snps, u32* __restrict__ n_het, u32* __restrict__ n_hom)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ind) return;
    const size_t ra = 2 * (ind_begin + i), rb = ra + 1;
    u32 ja = m_off[ra], jb = m_off[rb];
    const u32 ea = jb, eb = m_off[rb + 1];
    while (ja < ea || jb < eb) {
        const u64 x = jb >= eb ? m_pos[ja] : ja >= ea ? m_pos[jb] : (m_pos[ja] < m_pos[jb] ? m_pos[ja] : m_pos[jb]);
        u32 ma = 0, mb = 0;                                                             // the position is in the list of haplotype a / b
        while (ja < ea && m_pos[ja] == x) { ma = 1; ja++; }
        while (jb < eb && m_pos[jb] == x) { mb = 1; jb++; }
        for (u32 c = snp_begin + lower_bound_u64(pos + snp_begin, n_snps, x); c < snp_begin + n_snps && pos[c] == x; c++) {
            const u32 fa = (rm.word32(ra, c >> 5) >> (c & 31)) & 1u, fb = (rm.word32(rb, c >> 5) >> (c & 31)) & 1u;
            const u32 na = fa ^ ma, nb = fb ^ mb;
            const u32 dhet = (na ^ nb) - (fa ^ fb), dhom = (na & nb) - (fa & fb);       // +1, 0 or -1 (mod 2^32)
            if (dhet) atomicAdd(n_het + (c - snp_begin), dhet);
            if (dhom) atomicAdd(n_hom + (c - snp_begin), dhom);
        }
    }
}
#endif
