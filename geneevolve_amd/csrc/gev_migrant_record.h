// gev_migrant_record.h -- the packed migrant record of gev_export_size / gev_export_rows / gev_import_rows: its byte layout, once.
// Host only, no HIP and no context: tools/migrant_record_check.cpp compiles it alone.
//
// The record of n individuals is a sequence of sections, every one starting at a multiple of 16 bytes (the gap behind a section is
// padding nobody reads), in this order:
//   [counts]  u32[n][nchr][2 haplotypes][2]: the lengths (mutations, interval parts) of the lists of haplotype row 2i + h of
//             chromosome k, at index ((i * nchr + k) * 2 + h) * 2 + pass; pass 0: mutations, 1: interval parts
//   [sex]     u8[n]: Human::sex
//   [planes]  per chromosome k in ascending order: the 2n genotype rows of stride[k] bytes, row 2i + h behind row 2i + h - 1
//   [cv]      per phenotype p, and inside it per chromosome k (phenotype-major): the 2n CV rows of cv_row_bytes[p][k] bytes
//   [muts]    per chromosome k: the u64 mutation lists of the 2n rows, concatenated in row order (n_muts(k) entries)
//   [parts]   per chromosome k: the 32-byte gev_part interval lists likewise (n_parts(k) entries)
// A genotype row is the row as the pool holds it, i.e. before the row's own mutation list is applied: locus j is bit j % 8 of byte
// j / 8, and stride[k] is the chromosome's ceil(L / 8) bytes rounded up to a multiple of 128.  A CV row is u32 words: the first
// max(ceil(C / 32), 1) hold the alleles of the C causal variants, columns in ascending position (equal positions in file order);
// as many words again follow per bit of the root-population number (the smallest b with 2^b >= number of populations); the row is
// rounded up to 16 bytes.
// A chromosome the context does not hold (inactive: a locus-split population; both ends of an exchange hold the same set) has zero
// counts and takes no space in any section.  The [planes] section is empty unless genotype rows travel (dense state and
// gev_set_migrant_rows(1)); without interval tracking every parts count is zero and [parts] is empty.  The record ends behind the
// last section, rounded up to 16 bytes: `total`, what gev_export_size returns.
// A value that is to travel with the migrants adds one section to migrant_record_layout and one step each to export and import.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct MigrantRecord {
    static constexpr size_t MUT_BYTES = 8, PART_BYTES = 32;        // sizeof(u64), sizeof(gev_part)
    static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
    // the only place that knows where a count stands in the header
    static size_t count_index(size_t i, int nchr, int k, int h, int pass) { return ((i * nchr + k) * 2 + h) * 2 + pass; }
    static size_t n_counts(size_t n, int nchr) { return n * nchr * 4; }

    size_t n = 0; int nchr = 0, nphen = 0;
    const uint32_t* counts = nullptr;                              // borrowed: n_counts(n, nchr) entries that outlive the structure
    size_t counts_at = 0, sex_at = 0, total = 0;                   // byte offsets of the two fixed sections, bytes of the record
    std::vector<size_t> planes, cv, muts, parts, nmuts, nparts;    // per chromosome ([p * nchr + k] for cv): section starts, list entries

    size_t planes_at(int k) const { return planes[k]; }
    size_t cv_at(int p, int k) const { return cv[(size_t)p * nchr + k]; }
    size_t muts_at(int k) const { return muts[k]; }
    size_t parts_at(int k) const { return parts[k]; }
    size_t n_muts(int k) const { return nmuts[k]; }
    size_t n_parts(int k) const { return nparts[k]; }
    uint32_t count(size_t i, int k, int h, int pass) const { return counts[count_index(i, nchr, k, h, pass)]; }
    // exclusive offsets (2n + 1 of them, from `base`) of the haplotype rows of chromosome k; pass 0: mutations, 1: interval parts
    std::vector<uint32_t> row_offsets(int k, int pass, uint32_t base = 0) const
    {
        std::vector<uint32_t> off(2 * n + 1);
        off[0] = base;
        for (size_t i = 0; i < n; i++) for (int h = 0; h < 2; h++) off[2 * i + h + 1] = off[2 * i + h] + count(i, k, h, pass);
        return off;
    }
};

// active[nchr], stride[nchr] (bytes of a genotype row), cv_row_bytes[nphen * nchr] (phenotype-major), counts: see above
static inline MigrantRecord migrant_record_layout(size_t n, int nchr, int nphen, const uint8_t* active, bool rows_travel, const size_t* stride,
                                                  const size_t* cv_row_bytes, const uint32_t* counts)
{
    MigrantRecord r;
    r.n = n; r.nchr = nchr; r.nphen = nphen; r.counts = counts;
    r.nmuts.assign(nchr, 0); r.nparts.assign(nchr, 0);
    for (size_t i = 0; i < n; i++) for (int k = 0; k < nchr; k++) for (int h = 0; h < 2; h++) { r.nmuts[k] += r.count(i, k, h, 0); r.nparts[k] += r.count(i, k, h, 1); }
    size_t off = 0;
    auto place = [&off](size_t bytes) { const size_t at = off; off = MigrantRecord::al16(off + bytes); return at; };   // a section of 0 bytes takes no space
    r.counts_at = place(MigrantRecord::n_counts(n, nchr) * sizeof(uint32_t));
    r.sex_at = place(n);
    for (int k = 0; k < nchr; k++) r.planes.push_back(place(active[k] && rows_travel ? 2 * n * stride[k] : 0));
    for (int p = 0; p < nphen; p++) for (int k = 0; k < nchr; k++) r.cv.push_back(place(active[k] ? 2 * n * cv_row_bytes[(size_t)p * nchr + k] : 0));
    for (int k = 0; k < nchr; k++) r.muts.push_back(place(r.nmuts[k] * MigrantRecord::MUT_BYTES));
    for (int k = 0; k < nchr; k++) r.parts.push_back(place(r.nparts[k] * MigrantRecord::PART_BYTES));
    r.total = off;
    return r;
}
