"""gev_snp_trait_sums: per SNP and trait the sum of the trait's quanta weighted by the genotype and over the heterozygous individuals,
and the two genotype counts -- taken on the device from the current generation (geneevolve_amd/csrc/gev_traitsum.h: the SNP-major
plane of the LD calls against the traits' digits laid out in the plane's byte order, exact int8 matrix-core products, the individuals
split over workgroups).  The truth is numpy over gev_download_haps; the host build of the same arithmetic is held against it too.
Every comparison is exact."""
import os
import re

import numpy as np
import pytest

from geneevolve_amd import assoc, capi
from geneevolve_amd.host import Simulation, SyntheticConfig
from tests import helpers
from tests.snp_counts_inputs import random_rows
from tests.test_gpu_phenotypes import adjusted_beta
from tests.test_gpu_snp_counts import overlay_situations, unpacked
from tests.trait_sums_inputs import NAMES, Q_MAX, numpy_trait_sums, one_hot_traits, one_hot_value, random_quanta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# words of a SNP's row (32 individuals each) that one workgroup of the product sums, as built
SLICE_WORDS = int(re.search(r"#define\s+GEV_TS_SLICE_W\s+(\d+)u", open(os.path.join(ROOT, "geneevolve_amd", "csrc", "gev_traitsum.h")).read()).group(1))
SLICE_IND = 32 * SLICE_WORDS
# individuals: everybody, from inside a half word, a whole word on a word, one, from inside a word across a 4-word step, the last ones
IND = [(0, 333), (5, 200), (32, 32), (100, 1), (21, 129), (300, 33)]
# SNPs: everything, across the 64-SNP words of a haplotype row, the last one, 15, 63, 65 and 129
SNPS = [(0, 512), (63, 130), (511, 1), (56, 15), (1, 63), (127, 65), (300, 129)]
N_TRAITS = (1, 4, 5, 17)


def check(ctx, pop, chr, bits, q, s0, ns, i0, ni, what, rows=None):
    """the device against numpy and, with the packed rows, against the host build"""
    got = ctx.snp_trait_sums(pop, chr, q, s0, ns, i0, ni)
    want = numpy_trait_sums(bits, s0, ns, i0, ni, q)
    label = f"{what}: chr {chr} SNPs [{s0},+{ns}) individuals [{i0},+{ni}) {np.atleast_2d(q).shape[0]} traits"
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == (np.int64 if name.endswith("sum") else np.uint32) and g.shape == w.shape, f"{label}: {name}"
        assert np.array_equal(g, w), f"{label}: {name} differs at {np.argwhere(g != w)[:5].tolist()}"
    if rows is not None:
        host = ctx.L.dbg_trait_sums_host(rows, bits.shape[1], q, s0, ns, i0, ni)
        assert all(np.array_equal(g, h) for g, h in zip(got, host)), f"{label}: device and host build differ"
    return got


@pytest.fixture(scope="module", params=[None, 4], ids=["default segments", "64-byte segments"])
def awkward(request, gpu_lib):
    """333 individuals x 512 SNPs (hot map, mutations, three generations): 666 haplotypes = 10 words and 26 bits, three steps of the
    product's loop, the last one padded; its unpacked and packed rows"""
    seg_chunks = request.param
    old = os.environ.get("GEV_SEG_CHUNKS")
    if seg_chunks:
        os.environ["GEV_SEG_CHUNKS"] = str(seg_chunks)
    try:
        n, L = 333, 512
        cfg = SyntheticConfig(n, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.05, mut_per_row=2e-3, n_cv=20, seed=5)
        ctx = gpu_lib.create(1, 1, 1)
        cfg.apply_static(ctx)
        ctx.synth_founders(0, 0, 2 * n, 31); ctx.synth_cv_founders(0, 0, 0, 2 * n, 32)
        sim = Simulation(ctx, 4242, 1, True)
        sim.ras_initial_human_gen0(0, n)
        for _ in range(3):
            sim.next_generation_rm(0, n)
        if seg_chunks:
            assert ctx.plane_ptr(0, 0)[1] == 64, "64-byte segments"
    finally:
        if seg_chunks:
            if old is None:
                del os.environ["GEV_SEG_CHUNKS"]
            else:
                os.environ["GEV_SEG_CHUNKS"] = old
    rows = ctx.download_haps(0, 0)
    yield ctx, n, L, capi.unpack_rows(rows, L), rows
    ctx.close()


@pytest.mark.parametrize("i0", [0, 3, 16, 37], ids=lambda b: f"ind_begin {b}")
def test_one_hot_traits_tell_the_byte_order(awkward, i0):
    """for every position p of a 128-individual matrix step a trait whose only quantum sits at individual i0 + first + p, a different
    value with four non-zero digits at each: gsum[p][j] = g_pj q_p, so one misplaced byte of the trait operand is one wrong entry.  The
    first individual even and odd, on and off a half word and a word; the 128 positions at the range's begin and at its end"""
    ctx, n, L, bits, rows = awkward
    ni = n - i0
    vals = np.array([one_hot_value(p) for p in range(128)], dtype=np.int64)
    for first in (0, ni - 128):
        gsum, hetsum, het, hom = check(ctx, 0, 0, bits, one_hot_traits(ni, first), 0, L, i0, ni, f"one-hot from {first}", rows)
        g = bits[2 * (i0 + first):2 * (i0 + first + 128):2, :].astype(np.int64) + bits[2 * (i0 + first) + 1:2 * (i0 + first + 128):2, :]
        assert np.array_equal(gsum, g * vals[:, None]) and np.array_equal(hetsum, (g == 1) * vals[:, None])
        assert (g == 1).any(axis=1).all() and (g == 2).any(axis=1).all(), "every position is told apart by some SNP"


@pytest.mark.parametrize("chunk", [0, 7], ids=["byte budgets", "output chunk 7"])
def test_ranges_of_individuals_and_snps(awkward, chunk):
    """every range of individuals against every range of SNPs with 1, 4, 5 and 17 traits in turn; with gev_dbg_output_chunk(7) a pass
    takes 7 SNPs, so the ranges are walked in up to 74 passes whose results land side by side in the caller's matrices"""
    ctx, n, L, bits, rows = awkward
    rs = np.random.RandomState(60 + chunk)
    ctx.dbg_output_chunk(chunk)
    try:
        k = 0
        for i0, ni in IND:
            for s0, ns in SNPS:
                check(ctx, 0, 0, bits, random_quanta(rs, N_TRAITS[k % 4], ni), s0, ns, i0, ni, f"chunk {chunk}", rows); k += 1
    finally:
        ctx.dbg_output_chunk(0)


@pytest.mark.parametrize("n_traits", N_TRAITS)
def test_every_number_of_traits_on_everybody(awkward, n_traits):
    ctx, n, L, bits, rows = awkward
    q = random_quanta(np.random.RandomState(n_traits), n_traits, n)
    first = check(ctx, 0, 0, bits, q, 0, L, 0, n, "everybody", rows)
    again = ctx.snp_trait_sums(0, 0, q, 0, L, 0, n)
    assert all(np.array_equal(a, b) for a, b in zip(first, again)), "a repeat of the call gives the same integers"
    if n_traits == 1:
        check(ctx, 0, 0, bits, q[0], 0, L, 0, n, "one trait as a vector")


def test_no_trait_gives_the_snp_counter(awkward):
    ctx, n, L, bits, rows = awkward
    for i0, ni in IND:
        for s0, ns in SNPS[:4]:
            gsum, hetsum, het, hom = ctx.snp_trait_sums(0, 0, np.zeros((0, ni), dtype=np.int32), s0, ns, i0, ni)
            want = ctx.snp_genotype_counts(0, 0, s0, ns, i0, ni)
            assert gsum.shape == hetsum.shape == (0, ns) and np.array_equal(het, want[0]) and np.array_equal(hom, want[1])


def test_each_output_may_be_null_and_empty_requests(awkward):
    ctx, n, L, bits, rows = awkward
    f = ctx.L._f("snp_trait_sums")
    q = random_quanta(np.random.RandomState(2), 3, 200)
    want = numpy_trait_sums(bits, 70, 20, 5, 200, q)
    for k in range(4):
        out = [None] * 4
        out[k] = np.full(want[k].shape, 7, dtype=np.int64 if k < 2 else np.uint32)
        assert f(ctx.h, 0, 0, 70, 20, 5, 200, q, 3, *out) == 0
        assert np.array_equal(out[k], want[k]), NAMES[k]
    m = [np.full((3, 20), 7, dtype=np.int64) for _ in range(2)]; v = [np.full(20, 7, dtype=np.uint32) for _ in range(2)]
    outs = m + v
    assert f(ctx.h, 0, 0, 70, 0, 5, 200, q, 3, *outs) == 0 and all((a == 7).all() for a in m + v), "no SNP: nothing is touched"
    assert f(ctx.h, 0, 0, 70, 20, 5, 0, None, 3, *outs) == 0 and not any(a.any() for a in m + v), "no individual: zeros"
    assert f(ctx.h, 0, 0, 70, 20, 5, 200, q, 3, None, None, None, None) == 0


# ---- more individuals than one slice of the split --------------------------------------------------------------------------------------
def test_individuals_split_over_workgroups(gpu_lib):
    """20 000 individuals x 512 SNPs: a workgroup of the product sums a slice of GEV_TS_SLICE_W = 64 words of a SNP's row = 2048
    individuals (read from the header), so everybody is 10 slices whose partial sums meet in atomic adds; ranges that begin and end inside
    a slice, that straddle one slice edge, and that lie in the last slice.  Founders with every allele frequency from 0 to 1.  Quanta over
    the whole +-2^30: the sums reach 2^45, the digit sums 2^22"""
    assert SLICE_IND == 2048
    n, L = 20000, 512
    assert n >= 3 * SLICE_IND
    cfg = SyntheticConfig(n, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.02, n_cv=10, seed=8, with_mutation=False)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.upload_founders(0, 0, capi.pack_rows(random_rows(np.random.RandomState(21), n, L)), L)
    ctx.synth_cv_founders(0, 0, 0, 2 * n, 9)
    sim = Simulation(ctx, 77, 1, True)
    sim.ras_initial_human_gen0(0, n)
    sim.next_generation_rm(0, n)
    rows = ctx.download_haps(0, 0)
    bits = capi.unpack_rows(rows, L)
    rs = np.random.RandomState(5)
    for (i0, ni), nt in (((0, n), 5), ((3, n - 10), 4), ((SLICE_IND - 1, 2 * SLICE_IND + 2), 17), ((SLICE_IND - 40, 80), 1), ((n - 100, 100), 5)):
        check(ctx, 0, 0, bits, random_quanta(rs, nt, ni), 0, L, i0, ni, "20 000 individuals")
    extreme = np.where(rs.random_sample((2, n)) < 0.5, Q_MAX, -Q_MAX).astype(np.int32); extreme[1] = Q_MAX       # every digit sum as large as it gets
    check(ctx, 0, 0, bits, extreme, 100, 129, 0, n, "quanta at +-2^30")
    ctx.dbg_output_chunk(100)
    try:
        check(ctx, 0, 0, bits, random_quanta(rs, 5, n - 7), 3, 300, 7, n - 7, "20 000 individuals, passes of 100 SNPs")
    finally:
        ctx.dbg_output_chunk(0)
    q = random_quanta(rs, 3, 4500)
    host = gpu_lib.dbg_trait_sums_host(rows, L, q, 200, 40, 2000, 4500)
    assert all(np.array_equal(g, h) for g, h in zip(ctx.snp_trait_sums(0, 0, q, 200, 40, 2000, 4500), host)), "device and host build"
    ctx.close()


# ---- fixture replays -------------------------------------------------------------------------------------------------------------------
def founder_plane(ctx, pop, chr, bits, pos):
    """the rows without the mutation overlay: a haplotype's bit at a SNP whose position is in its mutation list is the founder's flipped"""
    muts, off = ctx.download_mutations(pop, chr)
    plane = bits.copy()
    for h in range(bits.shape[0]):
        cols = np.flatnonzero(np.isin(pos, muts[int(off[h]):int(off[h + 1])]))
        plane[h, cols] ^= 1
    return plane


@pytest.mark.parametrize("case", ["dense", "ex1mut"])
def test_trait_sums_of_replayed_fixtures(gpu_lib, oracle_lib, case):
    """the fixture's generations replayed through the library (ex1mut: mutation map and three chromosomes; dense: 434 of its mutations
    lie on SNPs, none of ex1mut's do).  At the last generation, for every chromosome: everybody and a sub-range, 5 traits.  In dense the
    overlay is at work: the counts of some SNPs differ from those of the rows without it"""
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
    rs = np.random.RandomState(12)
    moved = 0
    for ip in range(n_pop):
        n = ctx.pop_size(ip)
        first = ctx.snp_trait_sums(ip, 0, np.ones(n, dtype=np.int32))             # before anything else has asked for the population's rows
        for ic in range(nchr):
            L = ctx._nsnp[(ip, ic)]
            rows = ctx.download_haps(ip, ic)
            bits = capi.unpack_rows(rows, L)
            if ic == 0:
                assert np.array_equal(first[0][0], bits.sum(axis=0, dtype=np.int64)), "the first call"
            got = check(ctx, ip, ic, bits, random_quanta(rs, 5, n), 0, L, 0, n, case, rows)
            i0, ni = n // 4, n - n // 3
            ns = min(L, 300)
            check(ctx, ip, ic, bits, random_quanta(rs, 5, ni), (L - ns) // 2, ns, i0, ni, case, rows)
            plain = numpy_trait_sums(founder_plane(ctx, ip, ic, bits, fx[f"pop{ip}_chr{ic}_snp_pos"]), 0, L, 0, n, np.zeros((0, n)))
            moved += int(((got[2] != plain[2]) | (got[3] != plain[3])).sum())
    if case == "dense":
        assert moved >= 1, "a SNP whose counts the mutation overlay changes"
    if case == "ex1mut":
        assert nchr == 3
    ctx.close()


def test_trait_sums_under_the_mutation_overlay(gpu_lib):
    """the population of test_counts_under_the_mutation_overlay: mutations on SNPs whose founder bit was 1, on both haplotypes of an
    individual, repeated within a list, at positions that several SNP columns share"""
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
    assert a >= 1 and b >= 1 and c >= 1 and d >= 1
    rs = np.random.RandomState(3)
    for s0, ns in ((0, L), (10, 3), (301, 350)):
        check(ctx, 0, 0, bits, random_quanta(rs, 5, n), s0, ns, 0, n, "overlay")
        check(ctx, 0, 0, bits, random_quanta(rs, 4, 116), s0, ns, 17, 116, "overlay")
    ctx.close()


# ---- assoc.py on the device's phenotypes ---------------------------------------------------------------------------------------------------
def test_assoc_on_device_phenotypes(gpu_lib):
    """600 individuals x 2048 SNPs, two phenotypes computed on the device in generation 0 and after one generation of assortative
    mating; the floats of download_phenotypes through assoc.sums: the integers equal numpy's on the same quanta, and the slope, r^2, class
    means and F agree with a float64 regression on the floats within the quantisation (2^-31 of the largest deviation per individual)"""
    n, L = 600, 2048
    cfg = SyntheticConfig(n, L, chrom_bp=4_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=100, nphen=2, seed=6, vd=0.2)
    ctx = gpu_lib.create(1, 1, 2)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 51)
    for p in range(2):
        ctx.synth_cv_founders(0, p, 0, 2 * n, 52 + p)
    sim = Simulation(ctx, 4242, 1, True, track_pedigree=True, device_pedigree=True)
    sim.ras_initial_human_gen0(0, n)
    base = [(0.5, 0.1, 0.1, 0.2, 0.1), (0.4, 0.0, 0.2, 0.3, 0.1)]               # va, vd, vc, ve, vf
    beta = [1.0, 1.0]
    schemes = lambda: [b + (beta[p],) for p, b in enumerate(base)]
    sim.generation_phenotypes(0, 0, schemes(), 1)
    r = sim.phenotypes_result(0)
    for p in range(2):
        beta[p] = adjusted_beta(r["var"][p], base[p][4], 1)
    ctx.compute_selection(0, 0, "none", 0, 0, [1.0, 0.5], [1.0, 1.0], want=())
    sim.save_prev_gen(0)
    sim.next_generation_am_selected(0, n, 0.3, 0.1, True, "p", want_couples=True)
    sim.generation_phenotypes(0, 1, schemes(), 1)
    y = np.stack([ctx.download_phenotypes(0, p)["phen"] for p in range(2)])
    n = ctx.pop_size(0)                                                         # (what the couples bred)
    assert n >= 550 and y.shape == (2, n) and np.isfinite(y).all() and y.std(axis=1).min() > 0
    bits = unpacked(ctx, 0, 0)
    for (s0, ns), (i0, ni) in (((0, L), (0, n)), ((100, 333), (50, 500))):
        s = assoc.sums(ctx, 0, 0, y[:, i0:i0 + ni], snps=(s0, ns), ind=(i0, ni))
        q, scale, mean = assoc.quantise(y[:, i0:i0 + ni])
        want = numpy_trait_sums(bits, s0, ns, i0, ni, q)
        assert s.n_ind == ni and all(np.array_equal(g, w) for g, w in zip((s.gsum, s.hetsum, s.n_het, s.n_hom_alt), want))
        assert [int(v) for v in s.sum_q] == [int(v) for v in q.astype(np.int64).sum(axis=1)]
        add, gen = assoc.additive(s), assoc.genotypic(s)
        g = (bits[2 * i0:2 * (i0 + ni):2, s0:s0 + ns] + bits[2 * i0 + 1:2 * (i0 + ni):2, s0:s0 + ns]).astype(np.float64)
        poly = g.min(axis=0) != g.max(axis=0)
        assert poly.sum() > ns // 2 and np.array_equal(np.isnan(add.beta), np.broadcast_to(~poly, add.beta.shape))
        dg = g - g.mean(axis=0)
        for t in range(2):
            dy = y[t, i0:i0 + ni] - y[t, i0:i0 + ni].mean()
            sxx, sxy, syy = (dg * dg).sum(axis=0), dg.T @ dy, dy @ dy
            with np.errstate(divide="ignore", invalid="ignore"):
                assert np.allclose(add.beta[t][poly], (sxy / sxx)[poly], rtol=1e-6, atol=1e-9)
                assert np.allclose(add.r2[t][poly], (sxy * sxy / (sxx * syy))[poly], rtol=1e-6, atol=1e-12)
            for k in range(3):
                for j in np.flatnonzero(poly)[:40]:
                    cls = y[t, i0:i0 + ni][g[:, j] == k]
                    assert (len(cls) == 0 and np.isnan(gen.means[k, t, j])) or np.isclose(gen.means[k, t, j], cls.mean(), rtol=1e-8)
        assert np.isfinite(add.t[:, poly]).all() and np.isfinite(gen.F[:, poly]).all() and (gen.F[:, poly] >= 0).all()
    ctx.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_trait_sums_refusals(gpu_lib):
    n, L = 50, 300
    cfg = SyntheticConfig(n, L, nchr=2, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, n_cv=10, seed=2, with_mutation=False)
    q = np.zeros((2, n), dtype=np.int32)

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
    assert refused(lambda: ctx.snp_trait_sums(0, 0, q, 0, L, 0, n), "no resident genotype planes") == -2
    ctx.close()

    ctx = context(mine=(0,))
    assert refused(lambda: ctx.snp_trait_sums(0, 1, q, 0, 10, 0, n), "not active") == -2
    check(ctx, 0, 0, unpacked(ctx, 0, 0), q + 3, 0, L, 0, n, "one active chromosome")
    ctx.close()

    ctx = context(gen0=False)
    assert refused(lambda: ctx.snp_trait_sums(0, 0, q, 0, L, 0, n), "no current generation") == -2
    ctx.init_gen0(0, n, 77)
    bits = unpacked(ctx, 0, 1)
    rs = np.random.RandomState(1)

    def still_usable():
        check(ctx, 0, 1, bits, random_quanta(rs, 5, 40), 3, 100, 7, 40, "after a refusal")
    still_usable()
    assert refused(lambda: ctx.snp_trait_sums(0, 0, q, L - 1, 2, 0, n), "SNPs") == -1
    assert refused(lambda: ctx.snp_trait_sums(0, 0, q[:, :2], 0, L, n - 1, 2), "individuals") == -1
    for bad in (Q_MAX + 1, -Q_MAX - 1):
        q1 = q.copy(); q1[1, n - 1] = bad
        assert refused(lambda: ctx.snp_trait_sums(0, 0, q1, 0, L, 0, n), "quantum") == -1
    f = ctx.L._f("snp_trait_sums")
    out = np.zeros((2, L), dtype=np.int64)
    assert f(ctx.h, 0, 0, 0, L, 0, n, None, 2, out, None, None, None) == -1 and "null trait" in gpu_lib.last_error()
    still_usable()
    ctx.close()
    # more than 2^22 individuals: refused before anything is touched (the population itself is smaller, so the range is refused first
    # there; the bound is pinned on the host build, which takes the count of individuals as an argument)
    big = (1 << 22) + 1
    fh = gpu_lib._f("dbg_trait_sums_host")
    assert fh(None, 0, big, 10, 0, 1, 0, big, None, 1, None, None, None, None) == -5 and "at most" in gpu_lib.last_error()
