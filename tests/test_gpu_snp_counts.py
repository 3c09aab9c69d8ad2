"""gev_snp_genotype_counts: heterozygous / homozygous-alt counts per SNP taken on the device from the resident haplotype-major rows
(a bit-sliced positional popcount, geneevolve_amd/csrc/gev_snpcount.h) plus the sparse mutation overlay.  The truth is a numpy column
count over gev_download_haps, the route that is pinned on the reference's own .hap files; every comparison is exact."""
import numpy as np
import pytest

from geneevolve_amd import capi
from geneevolve_amd.host import Simulation, SyntheticConfig
from tests import helpers
from tests.snp_counts_inputs import F, numpy_counts

pytestmark = pytest.mark.gpu


def unpacked(ctx, pop, chr):
    return capi.unpack_rows(ctx.download_haps(pop, chr), ctx._nsnp[(pop, chr)])


def check_ranges(ctx, pop, chr, bits, snp_ranges, ind_ranges, what):
    """every SNP range x every individual range ([begin, end) pairs) against the numpy count over the same slice of `bits`"""
    for s0, s1 in snp_ranges:
        for i0, i1 in ind_ranges:
            het, hom = ctx.snp_genotype_counts(pop, chr, s0, s1 - s0, i0, i1 - i0)
            want = numpy_counts(bits[2 * i0:2 * i1], s0, s1 - s0)
            label = f"{what}: SNPs [{s0},{s1}) individuals [{i0},{i1})"
            assert het.dtype == np.uint32 and hom.dtype == np.uint32 and len(het) == len(hom) == s1 - s0, label
            assert np.array_equal(het, want[0]), f"{label}: n_het differs at {np.flatnonzero(het != want[0])[:5]}"
            assert np.array_equal(hom, want[1]), f"{label}: n_hom_alt differs at {np.flatnonzero(hom != want[1])[:5]}"


# ---- fixture replays -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dense", "ex1mut", "mig2", "mig3c"])
def test_counts_of_replayed_fixtures(gpu_lib, oracle_lib, case):
    """the fixture's generations replayed through the library (recorded couples, seeds and moves; ex1mut: mutation map and three
    chromosomes; mig2, mig3c: the last step is a migration, so the logical row order differs from the physical one and the count is
    the first call to ask for it).  At the last generation, for every population and chromosome: the whole range, three sub-ranges
    of SNPs and of individuals, and allele_freq."""
    fx = helpers.load_fixture(case)
    n_pop, nchr, nphen, ngen = int(fx["n_pop"]), int(fx["nchr"]), int(fx["nphen"]), int(fx["n_gen"])
    ctx = gpu_lib.create(n_pop, nchr, nphen)
    helpers.setup_static(ctx, fx)
    for ip, seed in enumerate(helpers.find_gen0_seeds(fx, oracle_lib)):
        ctx.init_gen0(ip, len(fx[f"g0_pop{ip}_sex"]), seed)
    for g in range(1, ngen + 1):
        for ip in range(n_pop):
            pre = f"g{g}_pop{ip}_"
            ms = fx[pre + "mut_seeds"]
            sex = ctx.reproduce(ip, fx[pre + "couples"], int(fx[pre + "seed_reproduce"]), ms if len(ms) else None)
            assert np.array_equal(sex, fx[pre + "sex"])
            ctx.compute_ad(ip)
        if f"g{g}_moves" in fx:
            ctx.migrate(helpers.derive_moves(fx, g))
    if case.startswith("mig"):
        assert f"g{ngen}_moves" in fx
    for ip in range(n_pop):
        n = ctx.pop_size(ip)
        first = ctx.snp_genotype_counts(ip, 0)                        # before anything else has asked for the population's rows
        for ic in range(nchr):
            L = ctx._nsnp[(ip, ic)]
            bits = unpacked(ctx, ip, ic)
            if ic == 0:
                want = numpy_counts(bits)
                assert np.array_equal(first[0], want[0]) and np.array_equal(first[1], want[1]), f"{case}: population {ip}, the first call"
            snps = [(0, L), (1, L - 1), (L // 3, 2 * L // 3 + 1), (L - 65, L)]
            inds = [(0, n), (1, n), (n // 3, n - 7), (n - 1, n)]
            check_ranges(ctx, ip, ic, bits, snps, inds, f"{case} population {ip} chromosome {ic}")
            het, hom = numpy_counts(bits)
            assert np.array_equal(ctx.allele_freq(ip, ic), (het.astype(np.float64) + 2.0 * hom) / (2.0 * n))
            sub = numpy_counts(bits[2 * 5:2 * (n - 3)], 7, L - 20)
            assert np.array_equal(ctx.allele_freq(ip, ic, 7, L - 20, 5, n - 8), (sub[0].astype(np.float64) + 2.0 * sub[1]) / (2.0 * (n - 8)))
    ctx.close()


# ---- shapes that can go wrong ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_chunks", [None, 4])
def test_counts_at_awkward_shapes(gpu_lib, monkeypatch, seg_chunks):
    """333 individuals x 5000 SNPs (40 chunks of 128 loci: a partly filled block of columns, a last chunk that ends before its 128th
    locus) bred on a hot map.  seg_chunks = 4: 64-byte segments, nearly every chunk of a row in a different unit.  Individual ranges
    at both ends, off by one, across the counter's overflow period; SNP ranges of one SNP at both ends, across a word edge, from the
    last bit of a chunk to the first of another.  gev_dbg_output_chunk must make no difference: the call stages nothing."""
    if seg_chunks:
        monkeypatch.setenv("GEV_SEG_CHUNKS", str(seg_chunks))
    n, L = 333, 5000
    cfg = SyntheticConfig(n, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.05, mut_per_row=2e-3, n_cv=20, seed=5)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 31); ctx.synth_cv_founders(0, 0, 0, 2 * n, 32)
    sim = Simulation(ctx, 4242, 1, True)
    sim.ras_initial_human_gen0(0, n)
    for _ in range(3):
        sim.next_generation_rm(0, n)
    if seg_chunks:
        assert ctx.plane_ptr(0, 0)[4] == 10 and ctx.plane_ptr(0, 0)[1] == 64, "ten 64-byte segments per row"
    bits = unpacked(ctx, 0, 0)
    inds = [(0, 1), (332, 333), (1, 333), (F - 1, 2 * F + 1), (0, n)]
    snps = [(0, 1), (4999, 5000), (31, 33), (127, 4097), (0, L)]
    check_ranges(ctx, 0, 0, bits, snps, inds, f"seg_chunks {seg_chunks}")
    ctx.dbg_output_chunk(7)
    check_ranges(ctx, 0, 0, bits, snps, inds, f"seg_chunks {seg_chunks}, output chunk 7")
    ctx.dbg_output_chunk(0)
    ctx.close()


# ---- mutation overlay ------------------------------------------------------------------------------------------------------------------
def overlay_situations(ctx, pos):
    """from the downloaded mutation lists and rows: (a) mutations at a SNP column whose founder bit was 1, (b) SNP positions mutated on
    both haplotypes of one individual, (c) positions repeated within one haplotype's list, (d) mutations at a position that two or
    more SNP columns share"""
    muts, off = ctx.download_mutations(0, 0)
    bits = unpacked(ctx, 0, 0)
    a = b = c = d = 0
    for i in range(ctx.pop_size(0)):
        lists = [muts[int(off[2 * i + h]):int(off[2 * i + h + 1])] for h in range(2)]
        for h, l in enumerate(lists):
            u, cnt = np.unique(l, return_counts=True)
            c += int((cnt > 1).sum())
            for x in u:
                cols = np.flatnonzero(pos == x)
                d += len(cols) > 1
                a += int((bits[2 * i + h, cols] == 0).sum())            # value = !founder: a 0 now was a founder 1
        b += int(np.isin(np.intersect1d(lists[0], lists[1]), pos).sum())
    return a, b, c, d, bits


def test_counts_under_the_mutation_overlay(gpu_lib):
    """150 individuals, 700 SNPs two base pairs apart on a 1400 bp chromosome, a mutation map hot enough (0.2 per 100 bp row and
    gamete) that in eight generations mutations land on SNPs, are inherited through both parents and are hit again; SNP columns 10-12,
    300-301 and 650-651 share a position.  Seed and rates were chosen with the CPU oracle under the same driver, where they give
    (a) 421, (b) 12, (c) 12, (d) 11; each must occur here, and the counts must equal the numpy truth in every range."""
    n, L = 150, 700
    cfg = SyntheticConfig(n, L, chrom_bp=1400, map_step=100, rec_per_row=0.05, mut_per_row=0.2, n_cv=8, seed=4)
    for k in (10, 11, 300, 650):
        cfg.snp_pos[k + 1] = cfg.snp_pos[k]
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 7); ctx.synth_cv_founders(0, 0, 0, 2 * n, 8)
    sim = Simulation(ctx, 4, 1, True)
    sim.ras_initial_human_gen0(0, n)
    for _ in range(8):
        sim.next_generation_rm(0, n)
    a, b, c, d, bits = overlay_situations(ctx, cfg.snp_pos)
    print(f"(a) cleared founder bits {a}, (b) both haplotypes {b}, (c) repeated positions {c}, (d) shared positions {d}")
    assert a >= 1 and b >= 1 and c >= 1 and d >= 1
    check_ranges(ctx, 0, 0, bits, [(0, L), (10, 13), (11, 12), (301, 651), (129, 700)], [(0, n), (0, 1), (17, 133), (n - 1, n)], "overlay")
    ctx.close()


# ---- larger population -----------------------------------------------------------------------------------------------------------------
def test_counts_of_many_individual_blocks(gpu_lib):
    """20 000 individuals x 4096 SNPs, one generation: one block of columns, many blocks of individuals that combine by atomics"""
    n, L = 20_000, 4096
    cfg = SyntheticConfig(n, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.01, mut_per_row=1e-3, n_cv=20, seed=6)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 41); ctx.synth_cv_founders(0, 0, 0, 2 * n, 42)
    sim = Simulation(ctx, 99, 1, True)
    sim.ras_initial_human_gen0(0, n)
    sim.next_generation_rm(0, n)
    het, hom = ctx.snp_genotype_counts(0, 0)
    words = ctx.download_haps(0, 0)
    a, b = words[0::2], words[1::2]
    want_het = np.unpackbits((a ^ b).view(np.uint8), axis=1, bitorder="little").sum(axis=0, dtype=np.uint32)
    want_hom = np.unpackbits((a & b).view(np.uint8), axis=1, bitorder="little").sum(axis=0, dtype=np.uint32)
    assert np.array_equal(het, want_het) and np.array_equal(hom, want_hom)
    popcount = int(np.unpackbits(words.view(np.uint8)).sum(dtype=np.int64))
    assert int(het.sum(dtype=np.int64) + 2 * hom.sum(dtype=np.int64)) == popcount
    # all but individuals 0, 1, 2 and n - 1: the whole count less what those four contribute
    out = np.r_[0:6, 2 * n - 2:2 * n]
    less = numpy_counts(capi.unpack_rows(words[out], L))
    h2, m2 = ctx.snp_genotype_counts(0, 0, 100, 3000, 3, n - 4)
    assert np.array_equal(h2, (want_het - less[0])[100:3100]) and np.array_equal(m2, (want_hom - less[1])[100:3100])
    ctx.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_snp_counts_refusals(gpu_lib):
    n, L = 50, 300
    cfg = SyntheticConfig(n, L, nchr=2, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, n_cv=10, seed=2, with_mutation=False)

    def refused(call, word):
        with pytest.raises(capi.GevError) as e:
            call()
        assert word in str(e.value), str(e.value)
        return e.value.code

    def context(dense=True, mine=(0, 1), gen0=True):
        ctx = gpu_lib.create(1, 2, 1)
        if not dense:
            ctx.set_dense_state(False)
        for c in range(2):
            ctx.set_rmap(0, c, cfg.rmap_bp, cfg.rmap_prob, cfg.bp_dist)
        for c in mine:
            ctx.set_snps(0, c, cfg.snp_pos)
            bp, a, d = cfg.cv[0][c]
            ctx.set_cvs(0, 0, c, bp, a, d, cfg.vd)
        for c in range(2):
            ctx.set_chr_active(c, c in mine)
        for c in mine:
            if dense:
                ctx.synth_founders(0, c, 2 * n, 50 + c)
            ctx.synth_cv_founders(0, 0, c, 2 * n, 60 + c)
        if gen0:
            ctx.init_gen0(0, n, 77)
        return ctx

    ctx = context(dense=False)
    assert refused(lambda: ctx.snp_genotype_counts(0, 0), "no resident genotype planes") == -2
    assert ctx.pop_size(0) == n
    ctx.close()

    ctx = context(mine=(0,))
    assert refused(lambda: ctx.snp_genotype_counts(0, 1, 0, 10), "not active") == -2
    want = numpy_counts(unpacked(ctx, 0, 0))
    got = ctx.snp_genotype_counts(0, 0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ctx.close()

    ctx = context(gen0=False)
    assert refused(lambda: ctx.snp_genotype_counts(0, 0, 0, L, 0, n), "no current generation") == -2
    ctx.init_gen0(0, n, 77)
    bits = unpacked(ctx, 0, 0)
    want = numpy_counts(bits)

    def still_usable():
        got = ctx.snp_genotype_counts(0, 0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    still_usable()
    assert refused(lambda: ctx.snp_genotype_counts(0, 0, L - 1, 2), "SNPs") == -1
    assert refused(lambda: ctx.snp_genotype_counts(0, 0, L + 1, 0), "SNPs") == -1
    assert refused(lambda: ctx.snp_genotype_counts(0, 0, 0, L, n - 1, 2), "individuals") == -1
    assert refused(lambda: ctx.snp_genotype_counts(0, 0, 0, L, n + 1, 0), "individuals") == -1
    still_usable()
    f = ctx.L._f("snp_genotype_counts")
    out = np.full(L, 7, dtype=np.uint32)
    for het, hom in ((None, out), (out, None), (None, None)):
        assert f(ctx.h, 0, 0, 0, L, 0, n, het, hom) == -1 and "null" in ctx.L.last_error()
    assert (out == 7).all()
    still_usable()
    # n_snps == 0 touches nothing (null vectors are fine); n_ind == 0 writes zeros
    assert f(ctx.h, 0, 0, 5, 0, 0, n, None, None) == 0
    assert f(ctx.h, 0, 0, L, 0, n, 0, None, None) == 0
    het, hom = ctx.snp_genotype_counts(0, 0, 3, 100, 10, 0)
    assert len(het) == 100 and not het.any() and not hom.any()
    het, hom = ctx.snp_genotype_counts(0, 0, 0, None, n, 0)
    assert len(het) == L and not het.any() and not hom.any()
    still_usable()
    check_ranges(ctx, 0, 1, unpacked(ctx, 0, 1), [(0, L), (299, 300)], [(0, n), (49, 50)], "second chromosome")
    ctx.close()
