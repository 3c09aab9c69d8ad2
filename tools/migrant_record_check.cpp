// migrant_record_check.cpp -- stand-alone check of geneevolve_amd/csrc/gev_migrant_record.h (the layout of the packed migrant record
// of gev_export_rows / gev_import_rows) against the format comment restated as one sequential cursor, host only.
// Build with sanitizers:  g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/migrant_record_check.cpp -o migrant_record_check
// Shapes: 0, 1, 3 and 17 individuals; 1, 2 and 5 chromosomes with none, the first, the last or a middle one inactive; 1 and 2
// phenotypes; genotype rows travelling or not; row strides that are multiples of 128 bytes and CV rows that are multiples of 16
// bytes, different per chromosome and phenotype; random list lengths with zeros among them, and all interval lengths zero (no
// interval tracking).  The counts are exactly sized, so a wrong index is a sanitizer report.
#include <cstdio>
#include "../geneevolve_amd/csrc/gev_migrant_record.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static unsigned long long n_checked = 0, n_bad = 0;
static void expect(bool ok, const char* what, size_t n, int nchr, int nphen, int inactive, bool rows, bool track)
{
    n_checked++;
    if (ok) return;
    n_bad++;
    printf("MISMATCH (%s): %zu individuals, %d chromosomes (inactive: %d), %d phenotypes, rows %d, intervals %d\n", what, n, nchr, inactive, nphen, (int)rows, (int)track);
}

static void check(size_t n, int nchr, int nphen, int inactive, bool rows, bool track)
{
    std::vector<uint8_t> active(nchr, 1);
    if (inactive >= 0) active[inactive] = 0;
    std::vector<size_t> stride(nchr), cvb((size_t)nphen * nchr);
    for (int k = 0; k < nchr; k++) stride[k] = 128 * (1 + rng() % 5);
    for (size_t j = 0; j < cvb.size(); j++) cvb[j] = 16 * (1 + rng() % 7);
    // u32[n][nchr][2][2], written with the strides of that array; zero for an inactive chromosome
    std::vector<uint32_t> counts(n * nchr * 4);
    for (size_t i = 0; i < n; i++) for (int k = 0; k < nchr; k++) for (int h = 0; h < 2; h++) {
        uint32_t* e = counts.data() + i * ((size_t)nchr * 4) + (size_t)k * 4 + (size_t)h * 2;
        e[0] = active[k] && rng() % 3 ? (uint32_t)(rng() % 9) : 0;
        e[1] = active[k] && track ? (uint32_t)(1 + rng() % 4) : 0;
    }
    const MigrantRecord r = migrant_record_layout(n, nchr, nphen, active.data(), rows, stride.data(), cvb.data(), counts.data());
    auto ex = [&](bool ok, const char* what) { expect(ok, what, n, nchr, nphen, inactive, rows, track); };

    // the format comment as one cursor: every section begins at the next multiple of 16 behind the one before it
    size_t cur = 0, prev_end = 0;
    auto section = [&](size_t at, size_t bytes, const char* what) {
        while (cur % 16) cur++;
        ex(at % 16 == 0, "alignment"); ex(at >= prev_end, "order"); ex(at == cur, what);
        cur += bytes; prev_end = at + bytes;
    };
    section(r.counts_at, n * nchr * 2 * 2 * 4, "counts");
    section(r.sex_at, n, "sex");
    for (int k = 0; k < nchr; k++) section(r.planes_at(k), active[k] && rows ? 2 * n * stride[k] : 0, "planes");
    for (int p = 0; p < nphen; p++) for (int k = 0; k < nchr; k++) section(r.cv_at(p, k), active[k] ? 2 * n * cvb[(size_t)p * nchr + k] : 0, "cv");
    std::vector<size_t> nm(nchr, 0), np(nchr, 0);
    for (int k = 0; k < nchr; k++) for (size_t row = 0; row < 2 * n; row++) {
        nm[k] += counts[(row / 2) * nchr * 4 + k * 4 + (row % 2) * 2]; np[k] += counts[(row / 2) * nchr * 4 + k * 4 + (row % 2) * 2 + 1];
    }
    for (int k = 0; k < nchr; k++) { ex(r.n_muts(k) == nm[k], "n_muts"); section(r.muts_at(k), nm[k] * 8, "muts"); }
    for (int k = 0; k < nchr; k++) { ex(r.n_parts(k) == np[k], "n_parts"); section(r.parts_at(k), np[k] * 32, "parts"); }
    while (cur % 16) cur++;
    ex(r.total == cur, "total");

    for (int k = 0; k < nchr; k++) for (int pass = 0; pass < 2; pass++) {
        const uint32_t base = pass ? 1000003u : 0u;
        const std::vector<uint32_t> off = r.row_offsets(k, pass, base);
        bool ok = off.size() == 2 * n + 1 && off[0] == base, same = true;
        uint32_t sum = base;
        for (size_t i = 0; i < n && ok; i++) for (int h = 0; h < 2; h++) {
            same = same && r.count(i, k, h, pass) == counts[i * nchr * 4 + k * 4 + h * 2 + pass];
            sum += r.count(i, k, h, pass);
            ok = ok && off[2 * i + h + 1] == sum;
        }
        ex(same, "count"); ex(ok, "row_offsets");
        ex(ok && off[2 * n] == base + (pass ? r.n_parts(k) : r.n_muts(k)), "row_offsets end");
    }
}

int main()
{
    const size_t ns[] = {0, 1, 3, 17};
    const int nchrs[] = {1, 2, 5};
    for (size_t n : ns)
        for (int nchr : nchrs) {
            std::vector<int> inactive = {-1, 0};                     // none, the first ...
            if (nchr > 1) inactive.push_back(nchr - 1);              // ... the last ...
            if (nchr > 2) inactive.push_back(nchr / 2);              // ... a middle one
            for (int ia : inactive)
                for (int nphen = 1; nphen <= 2; nphen++)
                    for (int rows = 0; rows < 2; rows++)
                        for (int track = 0; track < 2; track++) check(n, nchr, nphen, ia, rows != 0, track != 0);
        }
    printf("%llu checks, %llu mismatches\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
