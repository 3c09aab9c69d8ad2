// gev_outputs.h -- kernels that only the genotype output calls of gev_library.hip launch (gev_materialize*, gev_download_snp_major,
// gev_download_plink_matrix, gev_format_*): tiles from the interval state, SNP-major transposes, text and .bed formatting.  Included by
// gev_library.hip after gev_kernels.h, whose helpers (RowMap, lower_bound_u64) they use.
#pragma once

// K8: genotype tile from the ancestry intervals == Simulation::ras_convert_interval_to_hap_matrix (src/Simulation.cpp:1186-1230)
// restricted to haplotype rows [row0, row0+n_rows) x loci [s0, s0+ns): out[r][ii] = founder[part.hap_index][ii] for the part
// that contains pos[ii]; loci outside every part stay 0.  One thread per 32-bit word of the tile; the parts of a row are
// disjoint and ascending, so the first candidate is found by bisection on `en` and usually covers the whole word.
// `founder` holds the same loci range of every founder haplotype (bit j = locus s0 + j).  Mutations: k_tile_apply_mut.
__global__ void __launch_bounds__(256) k_materialize_tile(const u32* __restrict__ p_off, const gev_part* __restrict__ parts, size_t row0, size_t n_rows,
                                                          const u64* __restrict__ pos, u32 s0, u32 ns, const u32* __restrict__ founder, size_t founder_w32,
                                                          const u64* __restrict__ founder_row0 /* [n_pop+1]: rows of root population p are [row0[p], row0[p+1]) of `founder` */,
                                                          int n_pop, u32* __restrict__ out, size_t out_w32, u32* __restrict__ status)
{
    const u32 words = (ns + 31) / 32;
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_rows * words) return;
    const size_t r = q / words; const u32 w = (u32)(q % words);
    const u32 nb = min(32u, ns - 32u * w);
    const u64* wp = pos + s0 + 32u * w;                       // positions of this word's loci
    const u64 x0 = wp[0], x1 = wp[nb - 1];
    u32 lo = p_off[row0 + r], hi = p_off[row0 + r + 1];
    const u32 end = hi;
    while (lo < hi) { const u32 m = (lo + hi) >> 1; if (parts[m].en <= x0) lo = m + 1; else hi = m; }    // first part with en > x0
    u32 acc = 0;
    for (u32 i = lo; i < end && parts[i].st <= x1; i++) {
        const u64 st = parts[i].st, en = parts[i].en;
        u32 a = 0, b = 0;
        for (u32 t = 0; t < nb; t++) { a += wp[t] < st ? 1u : 0u; b += wp[t] < en ? 1u : 0u; }        // loci [a, b) lie in [st, en)
        if (b > a) {
            const u32 mask = (b - a == 32u) ? 0xffffffffu : (((1u << (b - a)) - 1u) << a);
            const u64 h = parts[i].hap_index;
            const int rp = parts[i].root_population;                                                  // founder panel of the part's ROOT population (:1204)
            if (rp < 0 || rp >= n_pop || h >= founder_row0[rp + 1] - founder_row0[rp]) { atomicOr(status, 1u); continue; }   // :1205-1209 "hap_index is not in range"
            acc |= founder[(founder_row0[rp] + h) * founder_w32 + w] & mask;
        }
    }
    out[r * out_w32 + w] = acc;
}
// mutation overlay of a tile: out bit = !unmutated bit at every tile locus whose position is in the row's mutation list (:1212-1216)
__global__ void __launch_bounds__(256) k_tile_apply_mut(const u32* __restrict__ plain, u32* __restrict__ out, size_t w32, size_t row0, size_t n_rows,
                                                        const u32* __restrict__ m_off, const u64* __restrict__ m_pos, const u64* __restrict__ pos, u32 s0, u32 ns)
{
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const u32* in = plain + r * w32; u32* o = out + r * w32;
    for (u32 j = m_off[row0 + r]; j < m_off[row0 + r + 1]; j++) {
        const u64 x = m_pos[j];
        u32 c = lower_bound_u64(pos + s0, ns, x);
        for (; c < ns && pos[s0 + c] == x; c++) {
            const u32 f = (in[c >> 5] >> (c & 31)) & 1u;
            if (f) o[c >> 5] &= ~(1u << (c & 31)); else o[c >> 5] |= (1u << (c & 31));
        }
    }
}
// ------------------------------------------------------------------------------------------
// K9: output packing.  The reference's .hap files are SNP-major text
// (format_hap::write_hap, src/format_hap.cpp:6-30); PLINK .bed is SNP-major 2-bit.  The resident
// plane is haplotype-major, so output = 64x64 bit-tile transposes (64 ballots per tile: lane b ends
// up with SNP 64*sw+b across 64 haplotypes), then the sparse mutation overlay, then formatting.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_transpose_tiles(const u64* __restrict__ plane /* flat rows, or null: */, RowMap rm /* segment pool */, size_t stride_w64, size_t n_rows, u32 L,
                                                         u32 snp_begin, u32 n_snps, u64* __restrict__ out, size_t out_stride_w64, u32 words_per_wave)
{
    const u32 lane = threadIdx.x & 63;
    const size_t hb = (size_t)blockIdx.x;                                   // block of 64 haplotype rows
    const u32 wave = blockIdx.y * 4 + (threadIdx.x >> 6);
    const u32 sw_first = snp_begin >> 6, sw_last = (snp_begin + n_snps - 1) >> 6;
    const u32 sw0 = sw_first + wave * words_per_wave;
    const size_t row = hb * 64 + lane;
    for (u32 sw = sw0; sw < sw0 + words_per_wave && sw <= sw_last; sw++) {
        const u64 v = row < n_rows ? (plane ? plane[row * stride_w64 + sw] : rm.word64(row, sw)) : 0ull;
        u64 mine = 0;
#pragma unroll 8
        for (u32 b = 0; b < 64; b++) {
            const u64 m = __ballot((v >> b) & 1ull);
            if (lane == b) mine = m;
        }
        const u32 snp = sw * 64 + lane;
        if (snp >= snp_begin && snp < snp_begin + n_snps && snp < L) out[(size_t)(snp - snp_begin) * out_stride_w64 + hb] = mine;
    }
}
// flip (snp, hap) where the SNP position is in the haplotype's mutation set: value = !founder (idempotent)
__global__ void __launch_bounds__(256) k_snpmajor_apply_mut(RowMap rm, size_t n_rows,
                                                            const u32* __restrict__ m_off, const u64* __restrict__ m_pos, const u64* __restrict__ pos, u32 L,
                                                            u32 snp_begin, u32 n_snps, unsigned long long* __restrict__ out, size_t out_stride_w64)
{
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    for (u32 j = m_off[r]; j < m_off[r + 1]; j++) {
        const u64 x = m_pos[j];
        u32 c = lower_bound_u64(pos, L, x);
        for (; c < L && pos[c] == x; c++) {
            if (c < snp_begin || c >= snp_begin + n_snps) continue;
            const u32 f = (rm.word32(r, c >> 5) >> (c & 31)) & 1u;
            unsigned long long* w = out + (size_t)(c - snp_begin) * out_stride_w64 + (r >> 6);
            const unsigned long long bit = 1ull << (r & 63);
            if (f) atomicAnd(w, ~bit); else atomicOr(w, bit);
        }
    }
}
// one .hap line per SNP: "b b b ... b \n" (digit + space per haplotype, then newline)
// The text is produced as a flat byte stream: thread t owns the aligned 16 bytes [16t, 16t+16) of the output (lines have odd
// lengths, so line-relative ownership would make every store misaligned), one 16-byte store per thread.
__global__ void __launch_bounds__(256) k_format_hap_text(const u64* __restrict__ snpmajor, size_t stride_w64, size_t n_rows, u32 n_snps, char* __restrict__ out)
{
    const size_t line_len = 2 * n_rows + 1, total = (size_t)n_snps * line_len;
    const size_t o = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (o >= total) return;
    size_t j = o / line_len, p = o % line_len;
    union { char ch[16]; uint4 v; } u;
    u64 word = 0; size_t word_at = ~(size_t)0;
#pragma unroll
    for (int b = 0; b < 16; b++) {
        char ch = ' ';
        if (o + b >= total) ch = 0;
        else if (p == 2 * n_rows) ch = '\n';
        else if (!(p & 1)) {
            const size_t h = p >> 1, at = j * stride_w64 + (h >> 6);
            if (at != word_at) { word = snpmajor[at]; word_at = at; }
            ch = (char)('0' + (int)((word >> (h & 63)) & 1ull));
        }
        u.ch[b] = ch;
        if (++p == line_len) { p = 0; j++; }
    }
    if (o + 16 <= total) *reinterpret_cast<uint4*>(out + o) = u.v;
    else for (int b = 0; b < 16 && o + b < total; b++) out[o + b] = u.ch[b];
}
// VCF genotype columns of one data line (format_vcf::write_vcf_file, src/format_vcf.cpp:55-59): per individual "\ta|b"
// (a, b = haplotype rows 2i, 2i+1 at this SNP), then '\n'; flat-stream layout as above
__global__ void __launch_bounds__(256) k_format_vcf_gt(const u64* __restrict__ snpmajor, size_t stride_w64, size_t n_ind, u32 n_snps, char* __restrict__ out)
{
    const size_t line_len = 4 * n_ind + 1, total = (size_t)n_snps * line_len;
    const size_t o = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (o >= total) return;
    size_t j = o / line_len, p = o % line_len;
    union { char ch[16]; uint4 v; } u;
    u64 word = 0; size_t word_at = ~(size_t)0;
#pragma unroll
    for (int b = 0; b < 16; b++) {
        char ch;
        if (o + b >= total) ch = 0;
        else if (p == 4 * n_ind) ch = '\n';
        else if ((p & 3) == 0) ch = '\t';
        else if ((p & 3) == 2) ch = '|';
        else {
            const size_t h = p >> 1, at = j * stride_w64 + (h >> 6);      // p = 4i+1 -> row 2i, p = 4i+3 -> row 2i+1
            if (at != word_at) { word = snpmajor[at]; word_at = at; }
            ch = (char)('0' + (int)((word >> (h & 63)) & 1ull));
        }
        u.ch[b] = ch;
        if (++p == line_len) { p = 0; j++; }
    }
    if (o + 16 <= total) *reinterpret_cast<uint4*>(out + o) = u.v;
    else for (int b = 0; b < 16 && o + b < total; b++) out[o + b] = u.ch[b];
}
// PLINK .ped genotype columns (format_plink::write_ped_map / write_ped01_map, src/format_plink.cpp:42-49 / :114-121):
// per individual  L x " a b"  then '\n', a/b = allele letters of haplotype 0/1 (al1 if the bit is set else al0; "1"/"0"
// when al0 == NULL).  `rows` = staged hap-major rows (mutations applied) of individuals [0, n_ind); same flat-stream layout.
__global__ void __launch_bounds__(256) k_format_ped_text(const u32* __restrict__ rows, size_t stride_w32, size_t n_ind, u32 L,
                                                         const char* __restrict__ al0, const char* __restrict__ al1, char* __restrict__ out)
{
    const size_t line_len = 4 * (size_t)L + 1, total = n_ind * line_len;
    const size_t o = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (o >= total) return;
    size_t i = o / line_len, p = o % line_len;
    union { char ch[16]; uint4 v; } u;
    u32 w0 = 0, w1 = 0; size_t word_at = ~(size_t)0;
#pragma unroll
    for (int b = 0; b < 16; b++) {
        char ch = ' ';
        if (o + b >= total) ch = 0;
        else if (p == 4 * (size_t)L) ch = '\n';
        else if (p & 1) {
            const u32 s = (u32)(p >> 2), hap = (u32)(p >> 1) & 1u;
            const size_t at = 2 * i * stride_w32 + (s >> 5);
            if (at != word_at) { w0 = rows[at]; w1 = rows[at + stride_w32]; word_at = at; }
            const u32 bit = ((hap ? w1 : w0) >> (s & 31)) & 1u;
            ch = al0 ? (bit ? al1[s] : al0[s]) : (char)('0' + bit);
        }
        u.ch[b] = ch;
        if (++p == line_len) { p = 0; i++; }
    }
    if (o + 16 <= total) *reinterpret_cast<uint4*>(out + o) = u.v;
    else for (int b = 0; b < 16 && o + b < total; b++) out[o + b] = u.ch[b];
}
// matrix_plink_ped of ras_convert_interval_to_format_plink (src/Simulation.cpp:1308-1362): bit 2*ii+ihap of row ih
__device__ __forceinline__ u64 spread_bits(u32 x)
{
    u64 v = x;
    v = (v | (v << 16)) & 0x0000ffff0000ffffull; v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
    v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;  v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}
__global__ void __launch_bounds__(256) k_interleave_haps(const u32* __restrict__ rows, size_t stride_w32, size_t n_ind, u32 words, u64* __restrict__ out, size_t out_stride_w64)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_ind * words) return;
    const size_t i = q / words, w = q % words;
    out[i * out_stride_w64 + w] = spread_bits(rows[2 * i * stride_w32 + w]) | (spread_bits(rows[(2 * i + 1) * stride_w32 + w]) << 1);
}
// PLINK .bed body, SNP-major: 2 bits per individual, A1 = allele 1: 00 = 1/1, 10 = heterozygous, 11 = 0/0, pad = 00
__global__ void __launch_bounds__(256) k_format_bed(const u64* __restrict__ snpmajor, size_t stride_w64, size_t n_people, u32 n_snps, uint8_t* __restrict__ out)
{
    const size_t bpl = (n_people + 3) / 4;
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (size_t)n_snps * bpl) return;
    const size_t j = q / bpl, by = q % bpl;
    const u32 bits = (u32)((snpmajor[j * stride_w64 + (by >> 3)] >> ((by & 7) * 8)) & 0xffull);     // haplotypes 8*by .. 8*by+7
    u32 o = 0;
    for (u32 i = 0; i < 4; i++) {
        if (by * 4 + i >= n_people) break;
        const u32 b0 = (bits >> (2 * i)) & 1u, b1 = (bits >> (2 * i + 1)) & 1u;
        const u32 code = (b0 & b1) ? 0u : ((b0 ^ b1) ? 2u : 3u);
        o |= code << (2 * i);
    }
    out[q] = (uint8_t)o;
}

// ------------------------------------------------------------------------------------------
// Simulation::ras_write_hap_to_interval_format (src/Simulation.cpp:1582-1639): one text line per PART of the CSR interval lists, in
// list order (gev_fmt_int.h has the line).  Lists lengthen with the run's age and differ from row to row, so the work is cut by part:
// a block takes INT_PARTS consecutive parts of the request [p0, p1) = the lists of haplotype rows [row0, row1), one thread each.  The
// rows of the block's first and last part are found by bisection in the offsets (uniform over the block), every thread then bisects
// between the two.  k_int_rows<false> measures the lines (lens: one byte each, bsum: the block's bytes), k_info_scan64 turns the
// block sums into 64-bit byte offsets, k_int_rows<true> formats again into LDS at the lines' offsets inside the block and stores the
// block's contiguous byte range 16 bytes at a time, as k_info_rows does.
// ------------------------------------------------------------------------------------------
#define INT_PARTS 256                        // parts per block, one thread each
#define INT_SCAN_BYTES 32u                   // the block scan's scratch sits in the dynamic region too, so that the staging area stays 16-byte aligned
#define INT_LDS_BYTES (16u + INT_PARTS * GEV_INT_LINE_MAX)
static_assert(INT_SCAN_BYTES + INT_LDS_BYTES <= 65536, "a block's lines are staged in 64 KiB");
static_assert(GEV_INT_LINE_MAX <= 255, "a line's length is kept in one byte");
struct IntNames { const unsigned char* bytes; const u32* offs; u64 n; };      // founder names of one root population: name i = bytes[offs[i], offs[i+1])
struct IntLdsSink {                          // bytes beyond `cap` are dropped, never written
    unsigned char* lds; u32 cap;
    __device__ __forceinline__ void put(u32 pos, u32 c) { if (pos < cap) lds[pos] = (unsigned char)c; }
};
// the last row r of [lo, hi] with poff[r] <= q (rows without parts share their offset with the next one)
__device__ __forceinline__ size_t int_row_of(const u32* __restrict__ poff, u64 q, size_t lo, size_t hi)
{
    while (lo < hi) { const size_t mid = (lo + hi + 1) >> 1; if ((u64)poff[mid] <= q) lo = mid; else hi = mid - 1; }
    return lo;
}
// blocks [blk0, blk0 + gridDim.x) of the request.  ids[(row >> 1) - id_ind0] = Human::ID of the row's individual.
// WRITE = false: lens[part - p0], bsum[block]; *flag |= 1 for a part whose root population or founder has no name (length 0).
// WRITE = true : boff[block] - out_base = offset of the block's first byte in `out` (16-byte aligned).
// Dynamic LDS: INT_SCAN_BYTES, and with WRITE INT_LDS_BYTES behind them
template <bool WRITE>
__global__ void __launch_bounds__(INT_PARTS) k_int_rows(const u32* __restrict__ poff, const gev_part* __restrict__ parts, size_t row0, size_t row1, u32 p0, u32 p1,
                                                        const int64_t* __restrict__ ids, size_t id_ind0, int chr_label, const IntNames* __restrict__ names, int n_pop, u32 blk0,
                                                        uint8_t* __restrict__ lens, u32* __restrict__ bsum, const u64* __restrict__ boff, u64 out_base, char* __restrict__ out,
                                                        u32* __restrict__ flag)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char int_dyn[];
    u32* scan_lds = reinterpret_cast<u32*>(int_dyn);
    unsigned char* int_lds = int_dyn + INT_SCAN_BYTES;
    const u32 t = threadIdx.x;
    const size_t blk = (size_t)blk0 + blockIdx.x;
    const u64 qa = (u64)p0 + (u64)blk * INT_PARTS, q = qa + t;                 // (the grid never reaches beyond p1: qa < p1)
    const u64 qb = qa + INT_PARTS - 1 < (u64)p1 - 1 ? qa + INT_PARTS - 1 : (u64)p1 - 1;
    const bool live = q < (u64)p1;
    u32 len = 0, nlen = 0;
    GevIntLine l; const unsigned char* name = nullptr;
    if (live) {
        const size_t ra = int_row_of(poff, qa, row0, row1 - 1), rb = int_row_of(poff, qb, ra, row1 - 1);
        const size_t r = int_row_of(poff, q, ra, rb);
        const gev_part p = parts[q];
        const int rp = p.root_population;
        const u64 k = p.hap_index >> 1;
        if (rp < 0 || rp >= n_pop || k >= names[rp].n) { if (!WRITE) atomicOr(flag, 1u); }
        else {
            const u32 o0 = names[rp].offs[k];
            name = names[rp].bytes + o0; nlen = names[rp].offs[k + 1] - o0;
            l.id1 = (u64)(ids[(r >> 1) - id_ind0] + 1); l.st = p.st; l.en = p.en; l.hap1 = p.hap_index + 1; l.root1 = (u32)(rp + 1); l.ihap = (u32)(r & 1u); l.chr_label = chr_label;
            len = WRITE ? (u32)lens[q - p0] : gev_int_line_len(l, nlen);
        }
    }
    u32 total;
    const u32 ex = block_exclusive_scan_256(len, scan_lds, total);
    if (!WRITE) {
        if (live) lens[q - p0] = (uint8_t)len;
        if (t == 0) bsum[blk] = total;
        return;
    }
    const u64 g0 = boff[blk] - out_base;
    const u32 a = (u32)(g0 & 15u);
    if (len) { IntLdsSink s{int_lds, INT_LDS_BYTES}; gev_int_line(s, a + ex, l, name, nlen); }
    __syncthreads();
    // the block's bytes sit at LDS [a, a + total) with a = g0 mod 16: LDS chunk k and the aligned 16 bytes of `out` at g0 - a + 16 k coincide
    const u32 end = a + total < INT_LDS_BYTES ? a + total : INT_LDS_BYTES;
    char* base = out + (g0 - a);
    for (u32 lo = t * 16u; lo < end; lo += INT_PARTS * 16u) {
        if (lo >= a && lo + 16u <= end) *reinterpret_cast<uint4*>(base + lo) = *reinterpret_cast<const uint4*>(int_lds + lo);
        else for (u32 b = lo < a ? a : lo; b < lo + 16u && b < end; b++) base[b] = (char)int_lds[b];       // the two ragged ends of the block's range
    }
}
