"""gev_ld_counts / gev_ld_scores: per pair of SNPs the haplotypes that carry allele 1 at both and the genotype product, per SNP the
allele count and the heterozygous / homozygous-alt individuals, and per SNP the LD score of its window as an integer sum of r^2
quanta -- taken on the device from the current generation (geneevolve_amd/csrc/gev_ldcount.h: SNP-major rows, one pass to a plane, exact
int8 matrix-core products, the band reduced in the product's epilogue).  The truth is numpy over gev_download_haps, the route that is
pinned on the reference's own .hap files; every comparison is exact."""
import os

import numpy as np
import pytest

from geneevolve_amd import capi, ld
from geneevolve_amd.host import Simulation, SyntheticConfig
from tests import helpers
from tests.ld_inputs import LDTruth, numpy_ld_counts, numpy_q40_reassociated, rounding_shares, structured_rows
from tests.pair_counts_inputs import tile_mode
from tests.snp_counts_inputs import random_rows
from tests.test_gpu_snp_counts import overlay_situations, unpacked

pytestmark = pytest.mark.gpu

NAMES = ("n11", "gg", "c_a", "het_a", "hom_a", "c_b", "het_b", "hom_b")
# (n_a, n_b, a_begin, b_begin), a_begin != b_begin: a swapped row / column map cannot pass the rectangular ones
BLOCKS = [(1, 1, 5, 200), (15, 17, 3, 100), (16, 16, 40, 7), (33, 129, 290, 11), (129, 33, 0, 300), (33, 129, 4967, 4871)]
IND = [(0, 333), (5, 200), (32, 32), (100, 1)]
Q1 = np.uint64(1 << 40)


def check_block(ctx, pop, chr_a, bits_a, a0, na, chr_b, bits_b, b0, nb, i0, ni, what):
    got = ctx.ld_counts(pop, chr_a, a0, na, chr_b, b0, nb, i0, ni)
    want = numpy_ld_counts(bits_a, a0, na, bits_b, b0, nb, i0, ni)
    label = f"{what}: a chr {chr_a} [{a0},+{na}) b chr {chr_b} [{b0},+{nb}) individuals [{i0},+{ni})"
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape, label
        assert np.array_equal(g, w), f"{label}: {name} differs at {np.argwhere(g != w)[:5].tolist()}"
    return got


def check_scores(ctx, pop, chr, truth, s0, ns, lo, hi, i0, ni, genotype, what):
    score, terms = ctx.ld_scores(pop, chr, lo, hi, s0, ns, i0, ni, genotype)
    want = truth.scores(s0, lo, hi, genotype)
    label = f"{what}: SNPs [{s0},+{ns}) individuals [{i0},+{ni}) {'genotype' if genotype else 'haplotype'} r2"
    assert score.dtype == np.uint64 and terms.dtype == np.uint32 and len(score) == len(terms) == ns, label
    assert np.array_equal(terms, want[1]), f"{label}: n_terms differs at {np.flatnonzero(terms != want[1])[:5].tolist()}"
    assert np.array_equal(score, want[0]), f"{label}: score_q40 differs at {np.flatnonzero(score != want[0])[:5].tolist()}"
    return score, terms


def around_a_monomorphic_snp(bits, i0, ni, ns, reach):
    """(s0, truth): a range of ns SNPs around a SNP that is monomorphic among individuals [i0, +ni), chosen from the rows alone, and the
    truth of every SNP within `reach` of it"""
    L = bits.shape[1]
    c = bits[2 * i0:2 * (i0 + ni)].sum(axis=0)
    mono = np.flatnonzero((c == 0) | (c == 2 * ni))
    assert len(mono), "a monomorphic SNP among the individuals"
    m = int(mono[len(mono) // 2])
    s0 = min(max(m - ns // 2, 0), L - ns)
    t0, t1 = max(s0 - reach, 0), min(s0 + ns + reach, L)
    return s0, LDTruth(bits, t0, t1 - t0, i0, ni)


# ---- shapes that can go wrong ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[None, 4], ids=["default segments", "64-byte segments"])
def awkward(request, gpu_lib):
    """the 333 x 5000 population of test_gpu_pair_counts (hot map, mutations, three generations) and its rows: 666 haplotypes = 10 words
    and 26 bits, three passes of the product's loop"""
    seg_chunks = request.param
    old = os.environ.get("GEV_SEG_CHUNKS")
    if seg_chunks:
        os.environ["GEV_SEG_CHUNKS"] = str(seg_chunks)
    try:
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
    finally:
        if seg_chunks:
            if old is None:
                del os.environ["GEV_SEG_CHUNKS"]
            else:
                os.environ["GEV_SEG_CHUNKS"] = old
    yield ctx, n, L, unpacked(ctx, 0, 0), cfg.snp_pos
    ctx.close()


def rectangular_blocks(awkward, chunk):
    ctx, n, L, bits, pos = awkward
    ctx.dbg_output_chunk(chunk)
    try:
        for i0, ni in IND:
            for na, nb, a0, b0 in BLOCKS:
                check_block(ctx, 0, 0, bits, a0, na, 0, bits, b0, nb, i0, ni, "awkward shapes")
    finally:
        ctx.dbg_output_chunk(0)


@pytest.mark.parametrize("chunk", [0, 7], ids=["byte budgets", "output chunk 7"])
def test_rectangular_blocks(awkward, chunk):
    rectangular_blocks(awkward, chunk)


@pytest.mark.parametrize("chunk", [0, 7], ids=["byte budgets", "output chunk 7"])
def test_rectangular_blocks_on_the_large_tiles(awkward, chunk):
    """the same blocks and individual ranges with the 128 x 128 instantiations forced (gev_dbg_bitprod_tiles(2)), which the compute-unit
    rule gives no block below about 2000 SNPs a side: one partly filled tile, down to one pair in it"""
    with tile_mode(awkward[0], 2) as t:
        rectangular_blocks(awkward, chunk)
        small, large = t.launched()
        assert small == 0 and (large == 2 * len(IND) * len(BLOCKS) if chunk == 0 else large > 0)


def blocks_of_333_snps_and_the_identities(awkward):
    ctx, n, L, bits, pos = awkward
    for i0, ni in IND:
        n11, gg, c, het, hom = check_block(ctx, 0, 0, bits, 100, 333, 0, bits, 100, 333, i0, ni, "self block")[:5]
        assert np.array_equal(np.diag(n11), c) and np.array_equal(np.diag(gg), het + 4 * hom)
        assert np.array_equal(n11, n11.T) and np.array_equal(gg, gg.T)
        check_block(ctx, 0, 0, bits, 50, 333, 0, bits, 4600, 333, i0, ni, "distant block")
    ctx.dbg_output_chunk(7)
    try:
        for i0, ni in IND:
            check_block(ctx, 0, 0, bits, 50, 333, 0, bits, 4600, 333, i0, ni, "output chunk 7")
    finally:
        ctx.dbg_output_chunk(0)


def test_blocks_of_333_snps_and_the_identities(awkward):
    """333 x 333 SNPs: three tiles a side, the last one partly filled.  Of a self block: symmetric, n11[j][j] = c_j, gg[j][j] = het + 4 hom"""
    blocks_of_333_snps_and_the_identities(awkward)


def test_blocks_of_333_snps_and_the_identities_on_the_large_tiles(awkward):
    """333 x 333 SNPs on tiles of 128 x 128: three tiles a side, the last one filled to 77"""
    with tile_mode(awkward[0], 2) as t:
        blocks_of_333_snps_and_the_identities(awkward)
        assert t.large_only()


def test_per_snp_vectors_equal_the_snp_counter(awkward):
    ctx, n, L, bits, pos = awkward
    for i0, ni in IND:
        for s0, ns in ((0, 333), (63, 130), (L - 1, 1)):
            c_a, het_a, hom_a, c_b, het_b, hom_b = ctx.ld_counts(0, 0, s0, ns, 0, 7, 20, i0, ni)[2:]
            het, hom = ctx.snp_genotype_counts(0, 0, s0, ns, i0, ni)
            assert np.array_equal(het_a, het) and np.array_equal(hom_a, hom) and np.array_equal(c_a, het + 2 * hom)
            het, hom = ctx.snp_genotype_counts(0, 0, 7, 20, i0, ni)
            assert np.array_equal(het_b, het) and np.array_equal(hom_b, hom) and np.array_equal(c_b, het + 2 * hom)


def test_each_output_may_be_null_and_empty_requests(awkward):
    ctx, n, L, bits, pos = awkward
    f = ctx.L._f("ld_counts")
    want = numpy_ld_counts(bits, 70, 20, bits, 500, 30, 5, 200)
    for k in range(8):
        out = [None] * 8
        out[k] = np.full(want[k].shape, 7, dtype=np.uint32)
        assert f(ctx.h, 0, 0, 70, 20, 0, 500, 30, 5, 200, *out) == 0
        assert np.array_equal(out[k], want[k]), NAMES[k]
    # n_ind == 0 writes zeros; n_a == 0 or n_b == 0 touches nothing
    m = np.full((20, 30), 7, dtype=np.uint32); v = np.full(30, 7, dtype=np.uint32)
    assert f(ctx.h, 0, 0, 70, 20, 0, 500, 30, 5, 0, m, None, None, None, None, v, None, None) == 0
    assert not m.any() and not v.any()
    m[:] = 7; v[:] = 7
    assert f(ctx.h, 0, 0, 70, 0, 0, 500, 30, 5, 200, m, None, None, None, None, v, None, None) == 0
    assert f(ctx.h, 0, 0, 70, 20, 0, L, 0, 5, 200, m, None, v, None, None, None, None, None) == 0
    assert (m == 7).all() and (v == 7).all()
    lo, hi = ld.windows_by_count(L, 70, 20, 3)
    truth = LDTruth(bits, 60, 40, 5, 200).scores(70, lo, hi, True)
    fs = ctx.L._f("ld_scores")
    score = np.zeros(20, dtype=np.uint64); terms = np.zeros(20, dtype=np.uint32)
    assert fs(ctx.h, 0, 0, 70, 20, lo, hi, 5, 200, 1, score, None) == 0 and np.array_equal(score, truth[0])
    assert fs(ctx.h, 0, 0, 70, 20, lo, hi, 5, 200, 1, None, terms) == 0 and np.array_equal(terms, truth[1])
    score[:] = 7
    assert fs(ctx.h, 0, 0, 70, 20, lo, hi, 5, 0, 1, score, terms) == 0 and not score.any() and not terms.any()
    score[:] = 7
    assert fs(ctx.h, 0, 0, 70, 0, None, None, 5, 200, 1, score, None) == 0 and (score == 7).all()


def ld_scores_by_count(awkward, genotype):
    ctx, n, L, bits, pos = awkward
    for i0, ni in IND:
        s0, truth = around_a_monomorphic_snp(bits, 32, 32, 90, 300)
        if (i0, ni) != (32, 32):
            truth = LDTruth(bits, truth.s0, truth.ns, i0, ni)
        for chunk in (0, 7):
            ctx.dbg_output_chunk(chunk)
            try:
                for w in (0, 1, 50, 300):
                    lo, hi = ld.windows_by_count(L, s0, 90, w)
                    score, terms = check_scores(ctx, 0, 0, truth, s0, 90, lo, hi, i0, ni, genotype, f"w = {w}, chunk {chunk}")
                    poly = truth.poly[genotype][s0 - truth.s0:s0 - truth.s0 + 90]
                    if w == 0:
                        assert np.array_equal(score, np.where(poly, Q1, np.uint64(0))) and np.array_equal(terms, poly)
                    elif (i0, ni) == (32, 32):
                        assert truth.meaningful(s0, lo, hi, genotype), "a monomorphic and a polymorphic SNP, a quantum strictly between 0 and 2^40"
                        assert (~poly).any() and poly.any()
            finally:
                ctx.dbg_output_chunk(0)
    # the chromosome's two ends, where the windows are cut
    truth = LDTruth(bits, 0, 400, 5, 200)
    lo, hi = ld.windows_by_count(L, 0, 100, 300)
    check_scores(ctx, 0, 0, truth, 0, 100, lo, hi, 5, 200, genotype, "the first SNPs")
    truth = LDTruth(bits, L - 400, 400, 5, 200)
    lo, hi = ld.windows_by_count(L, L - 100, 100, 300)
    check_scores(ctx, 0, 0, truth, L - 100, 100, lo, hi, 5, 200, genotype, "the last SNPs")


@pytest.mark.parametrize("genotype", [False, True], ids=["haplotype r2", "genotype r2"])
def test_ld_scores_by_count(awkward, genotype):
    """w = 0, 1, 50, 300 on a sub-range of 90 SNPs whose windows reach outside it; among individuals (32, 32) the range lies around a
    monomorphic SNP, so the windows hold both kinds and the zero rule is at work"""
    ld_scores_by_count(awkward, genotype)


@pytest.mark.parametrize("genotype", [False, True], ids=["haplotype r2", "genotype r2"])
def test_ld_scores_by_count_on_the_large_tiles(awkward, genotype):
    """the score epilogue of the 128 x 128 instantiations (its own fragment loops, row reduction and atomics) on the same windows: of
    one SNP (w = 0), with an empty band on one side of the tile, around a monomorphic SNP, cut at the chromosome's ends"""
    with tile_mode(awkward[0], 2) as t:
        ld_scores_by_count(awkward, genotype)
        assert t.large_only()


def ld_scores_by_distance(awkward, genotype):
    ctx, n, L, bits, pos = awkward
    s0, truth = around_a_monomorphic_snp(bits, 32, 32, 150, 200)
    step = int(pos[1] - pos[0])
    for dist in (0, step, 37 * step + 1, 200 * step):
        lo, hi = ld.windows_by_distance(pos, s0, 150, dist)
        assert (hi - lo).max() <= 2 * (dist // step) + 1
        check_scores(ctx, 0, 0, truth, s0, 150, lo, hi, 32, 32, genotype, f"distance {dist}")
        if dist > step:
            assert truth.meaningful(s0, lo, hi, genotype)
    # uneven windows: a map whose steps vary, the windows of neighbours of very different widths
    rs = np.random.RandomState(9)
    uneven = np.cumsum(rs.choice([0, 1, 1, 3, 10, 200], size=L)).astype(np.uint64)
    lo, hi = ld.windows_by_distance(uneven, s0, 150, 150)
    lo, hi = np.maximum(lo, truth.s0).astype(np.uint32), np.minimum(hi, truth.s0 + truth.ns).astype(np.uint32)
    assert len(set((hi - lo).tolist())) > 10
    check_scores(ctx, 0, 0, truth, s0, 150, lo, hi, 32, 32, genotype, "uneven map")
    assert truth.meaningful(s0, lo, hi, genotype)


@pytest.mark.parametrize("genotype", [False, True], ids=["haplotype r2", "genotype r2"])
def test_ld_scores_by_distance(awkward, genotype):
    ld_scores_by_distance(awkward, genotype)


@pytest.mark.parametrize("genotype", [False, True], ids=["haplotype r2", "genotype r2"])
def test_ld_scores_by_distance_on_the_large_tiles(awkward, genotype):
    """... and on windows by distance, the uneven map included"""
    with tile_mode(awkward[0], 2) as t:
        ld_scores_by_distance(awkward, genotype)
        assert t.large_only()


# ---- more haplotype words than one pass of the loop, and not a multiple of its step -----------------------------------------------------
def test_many_haplotype_words(gpu_lib):
    """4100 individuals x 300 SNPs: 8200 haplotypes = 128 words and 8 bits, so 129 words padded to 132.  The founders are uploaded with
    every allele frequency from 0 to 1, so that monomorphic SNPs occur even among thousands"""
    n, L = 4100, 300
    cfg = SyntheticConfig(n, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.02, n_cv=10, seed=8, with_mutation=False)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.upload_founders(0, 0, capi.pack_rows(random_rows(np.random.RandomState(21), n, L)), L)
    ctx.synth_cv_founders(0, 0, 0, 2 * n, 9)
    sim = Simulation(ctx, 77, 1, True)
    sim.ras_initial_human_gen0(0, n)
    sim.next_generation_rm(0, n)
    bits = unpacked(ctx, 0, 0)
    for i0, ni in ((0, n), (3, 4090), (4064, 36)):
        check_block(ctx, 0, 0, bits, 0, L, 0, bits, 0, L, i0, ni, "4100 individuals")
        check_block(ctx, 0, 0, bits, 7, 129, 0, bits, 150, 33, i0, ni, "4100 individuals")
    for genotype in (False, True):
        truth = LDTruth(bits, 0, L, 0, n)
        lo, hi = ld.windows_by_count(L, 0, L, 50)
        check_scores(ctx, 0, 0, truth, 0, L, lo, hi, 0, n, genotype, "4100 individuals")
        assert truth.meaningful(0, lo, hi, genotype)
        lo, hi = ld.windows_by_count(L, 100, 150, L)
        check_scores(ctx, 0, 0, truth, 100, 150, lo, hi, 0, n, genotype, "4100 individuals, the whole chromosome")
    ctx.close()


# ---- the tiles of 128 x 128 ----------------------------------------------------------------------------------------------------------------
def test_blocks_and_bands_wide_enough_for_the_large_tiles(gpu_lib):
    """The product takes tiles of 128 x 128 where they give every compute unit work, of 64 x 64 otherwise; with the 256 compute units of an
    MI355X a block of 2100 x 2100 SNPs (17 x 17 large tiles) launches on the large ones alone and a band of 1500 SNPs to either side of
    4096 SNPs (644 large tiles in the first sub-block of 4096 SNPs, 68 in the second: one call, both tile sizes) on both, which the
    launch counters of gev_dbg_bitprod_tiles assert; the 2100 x 2100 block once more with the small tiles forced is a grid of 33 x 33 of
    them.  Then the walk at its real side, byte budgets alone: SNPs (0, 4200) x (700, 4300) are one sub-block of 4096 x 4096 on large
    tiles and the ragged remainders 4096 x 204, 104 x 4096 and 104 x 204 on small ones, copied out at a pitch of 4300 with side B's
    vectors at offset 4096; scores of all 5000 SNPs at w = 1500 are block rows of 4096 and 904 SNPs, the second with windows, scores
    and a band of its own.  40 individuals x 5000 SNPs, founders with every allele frequency from 0 to 1"""
    n, L = 40, 5000
    cfg = SyntheticConfig(n, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.05, n_cv=10, seed=6, with_mutation=False)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.upload_founders(0, 0, capi.pack_rows(random_rows(np.random.RandomState(22), n, L)), L)
    ctx.synth_cv_founders(0, 0, 0, 2 * n, 9)
    sim = Simulation(ctx, 78, 1, True)
    sim.ras_initial_human_gen0(0, n)
    sim.next_generation_rm(0, n)
    bits = unpacked(ctx, 0, 0)
    with tile_mode(ctx, 0) as t:
        for i0, ni in ((0, n), (3, 33)):
            check_block(ctx, 0, 0, bits, 0, 2100, 0, bits, 2500, 2100, i0, ni, "2100 x 2100 SNPs")
            assert t.launched() == (0, 2), "17 x 17 large tiles are more than the compute units: n11 and gg on the large tiles, and nothing else"
        check_block(ctx, 0, 0, bits, 2800, 2200, 0, bits, 1, 2049, 3, 33, "2200 x 2049 SNPs")
        assert t.launched() == (0, 2)
    with tile_mode(ctx, 1) as t:
        check_block(ctx, 0, 0, bits, 0, 2100, 0, bits, 2500, 2100, 3, 33, "2100 x 2100 SNPs, small tiles")
        assert t.launched() == (2, 0)
    truth = LDTruth(bits, 0, L, 3, 33)
    with tile_mode(ctx, 0) as t:
        # sub-blocks of 4096 SNPs a side, each matrix and vector against its slice of the truth
        got = list(ctx.ld_counts(0, 0, 0, 4200, 0, 700, 4300, 3, 33))
        assert t.launched() == (6, 2), "n11 and gg: one sub-block of 32 x 32 large tiles, three remainders on small ones"
        for k, (name, w) in enumerate(zip(NAMES, truth.block(0, 4200, 700, 4300))):
            assert got[k].dtype == np.uint32 and got[k].shape == w.shape, name
            assert np.array_equal(got[k], w), f"4200 x 4300 SNPs: {name} differs at {np.argwhere(got[k] != w)[:5].tolist()}"
            got[k] = None
        lo, hi = ld.windows_by_count(L, 0, 4096, 1500)
        for genotype in (False, True):
            check_scores(ctx, 0, 0, truth, 0, 4096, lo, hi, 3, 33, genotype, "w = 1500")
            small, large = t.launched()
            assert small == 1 and large == 1, "the band of the first sub-block on large tiles, of the second on small ones"
            assert truth.meaningful(0, lo, hi, genotype)
        # two block rows of SNPs
        lo, hi = ld.windows_by_count(L, 0, L, 1500)
        for genotype in (False, True):
            check_scores(ctx, 0, 0, truth, 0, L, lo, hi, 3, 33, genotype, "w = 1500, all 5000 SNPs")
            small, large = t.launched()
            assert small + large == 3 and small >= 1 and large >= 1, (small, large)
    ctx.close()


# ---- counts so large that every operation of the quantum rounds -----------------------------------------------------------------------------
def test_quanta_whose_products_round(gpu_lib):
    """32 000 individuals x 96 SNPs in strong LD (structured_rows), generation 0, individuals (0, 32000) and (3, 31965), both kinds of
    r^2, w = 20 and the whole chromosome, tiles by compute units (64 x 64 here) and 128 x 128 forced, so that both score epilogues
    round.  In every other device test n_ind <= 4100, so |num| and the denominators stay below 2^24.1, num^2 and den_j den_k are exact
    doubles and only the quotient rounds; here the largest num^2 is near 2^60.  Asserted on the downloaded rows: of the in-window terms
    with a quantum strictly between 0 and 2^40, num^2 is no double in at least 0.10 and den_j den_k in at least 0.10.  Measured:
    num^2 0.32 - 0.44, den_j den_k 0.78 - 0.85 (generation 0 keeps the founders' rows, so these are the shares of test_ld_cpu.py's
    host test).  Products or a quotient formed in less than a double, or a score summed in another type, differ here; another order
    of the same double operations shows in about one term in 10^5 and takes the million terms of the test below.  (double)num and
    (double)den stay exact below 2^27 haplotypes: those conversions are pinned on the host alone (test_ld_cpu.test_quantum_alone)"""
    n, L = 32000, 96
    cfg = SyntheticConfig(n, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.05, n_cv=10, seed=6, with_mutation=False)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.upload_founders(0, 0, capi.pack_rows(structured_rows(np.random.RandomState(31), n, L)), L)
    ctx.synth_cv_founders(0, 0, 0, 2 * n, 9)
    ctx.init_gen0(0, n, 81)
    bits = unpacked(ctx, 0, 0)
    for i0, ni in ((0, n), (3, 31965)):
        truth = LDTruth(bits, 0, L, i0, ni)
        windows = [ld.windows_by_count(L, 0, L, w) for w in (20, L)]
        for genotype in (False, True):
            for lo, hi in windows:
                nn, dd = rounding_shares(truth, 0, lo, hi, genotype)
                print(f"individuals [{i0},+{ni}) genotype {genotype} windows of {int((hi - lo).max())}: num^2 rounds in {nn:.3f} of the terms, den_j den_k in {dd:.3f}")
                assert truth.meaningful(0, lo, hi, genotype)
                assert nn >= 0.10 and dd >= 0.10, (i0, ni, genotype, nn, dd)
        for mode in (0, 2):
            with tile_mode(ctx, mode) as t:
                got = ctx.ld_counts(0, 0, 0, L, 0, 0, L, i0, ni)
                for name, g, w in zip(NAMES, got, truth.counts):
                    assert np.array_equal(g, w), f"individuals [{i0},+{ni}) tile mode {mode}: {name} differs at {np.argwhere(g != w)[:5].tolist()}"
                for genotype in (False, True):
                    for lo, hi in windows:
                        check_scores(ctx, 0, 0, truth, 0, L, lo, hi, i0, ni, genotype, f"tile mode {mode}")
                assert t.launched() == ((0, 6) if mode == 2 else (6, 0))
    ctx.close()


def test_quanta_that_tell_the_order_of_the_operations(gpu_lib):
    """The same founders with 1024 SNPs, individuals (3, 31965), the whole chromosome as every SNP's window: a million terms a kind.
    A quantum keeps 40 bits behind the point of an r^2 of 53, so r^2 formed as (x / dj) * (x / dk) shows in about one term in 10^5
    once the products round, and in none of the 36 864 terms of the test above (counted in numpy).  Here it does: asserted of the
    input, the reassociated form moves at least 3 scores of either kind (measured: 12 of haplotype r^2, 6 of genotype r^2), so equal
    scores say that the device forms the quotient of the two rounded products.  Tiles by compute units and 128 x 128 forced"""
    n, L, i0, ni = 32000, 1024, 3, 31965
    cfg = SyntheticConfig(n, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.05, n_cv=10, seed=6, with_mutation=False)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.upload_founders(0, 0, capi.pack_rows(structured_rows(np.random.RandomState(31), n, L)), L)
    ctx.synth_cv_founders(0, 0, 0, 2 * n, 9)
    ctx.init_gen0(0, n, 81)
    truth = LDTruth(unpacked(ctx, 0, 0), 0, L, i0, ni)
    lo, hi = ld.windows_by_count(L, 0, L, L)
    for genotype in (False, True):
        want = truth.scores(0, lo, hi, genotype)
        other = truth.scores(0, lo, hi, genotype, q=truth.quanta(genotype, numpy_q40_reassociated))
        moved = int((other[0] != want[0]).sum())
        print(f"genotype {genotype}: (x / dj) * (x / dk) moves {moved} of {L} scores")
        assert moved >= 3 and np.array_equal(other[1], want[1])
        for mode in (0, 2):
            with tile_mode(ctx, mode) as t:
                check_scores(ctx, 0, 0, truth, 0, L, lo, hi, i0, ni, genotype, f"tile mode {mode}")
                assert t.launched() == ((0, 1) if mode == 2 else (1, 0))
    ctx.close()


# ---- fixture replays -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ex1mut", "mig2"])
def test_ld_of_replayed_fixtures(gpu_lib, oracle_lib, case):
    """the fixture's generations replayed through the library (ex1mut: mutation map and three chromosomes, so a block between two
    chromosomes; mig2: the last step is a migration, so the logical row order differs from the physical one and the LD call is the
    first to ask for it).  At the last generation, for every population: blocks and LD scores of every chromosome through ld.py"""
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
        L0 = ctx._nsnp[(ip, 0)]
        first = ctx.ld_counts(ip, 0, 0, min(L0, 200), 0, 0, min(L0, 200))          # before anything else has asked for the population's rows
        rows = [unpacked(ctx, ip, ic) for ic in range(nchr)]
        for name, g, w in zip(NAMES, first, numpy_ld_counts(rows[0], 0, min(L0, 200), rows[0], 0, min(L0, 200), 0, n)):
            assert np.array_equal(g, w), f"{case}: population {ip}, the first call, {name}"
        for ic in range(nchr):
            L = ctx._nsnp[(ip, ic)]
            ns = min(L, 300)
            s0 = (L - ns) // 2
            i0, ni = n // 4, n - n // 3
            check_block(ctx, ip, ic, rows[ic], s0, ns, ic, rows[ic], 0, min(L, 150), 0, n, f"{case} population {ip}")
            jc = (ic + 1) % nchr
            if jc != ic:
                Lb = ctx._nsnp[(ip, jc)]
                check_block(ctx, ip, ic, rows[ic], s0, min(ns, 129), jc, rows[jc], Lb - min(Lb, 70), min(Lb, 70), i0, ni, f"{case} population {ip}, two chromosomes")
                counts = ld.counts(ctx, ip, ic, (s0, 40), jc, (0, min(Lb, 50)), (i0, ni))
                want = numpy_ld_counts(rows[ic], s0, 40, rows[jc], 0, min(Lb, 50), i0, ni)
                assert all(np.array_equal(g, w) for g, w in zip(counts[1:], want))
                r2 = ld.r2_haplotype(counts)
                assert np.nanmax(r2) <= 1.0 and np.array_equal(np.isnan(r2), ((want[2] == 0) | (want[2] == 2 * ni))[:, None] | ((want[5] == 0) | (want[5] == 2 * ni))[None, :])
            truth = LDTruth(rows[ic], 0, L, i0, ni) if L <= 1500 else LDTruth(rows[ic], max(s0 - 50, 0), min(ns + 100, L - max(s0 - 50, 0)), i0, ni)
            for genotype in (False, True):
                s = ld.ld_scores(ctx, ip, ic, w=50, snp_begin=s0, n_snps=ns, ind=(i0, ni), genotype=genotype)
                want = truth.scores(s0, *ld.windows_by_count(L, s0, ns, 50), genotype)
                assert np.array_equal(s.score_q40, want[0]) and np.array_equal(s.n_terms, want[1]), f"{case} population {ip} chromosome {ic}"
    if case == "ex1mut":
        assert nchr == 3
    ctx.close()


# ---- mutation overlay ------------------------------------------------------------------------------------------------------------------
def test_ld_under_the_mutation_overlay(gpu_lib):
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
    for a0, na, b0, nb in ((0, L, 0, L), (10, 3, 299, 4), (301, 350, 0, 129)):
        check_block(ctx, 0, 0, bits, a0, na, 0, bits, b0, nb, 0, n, "overlay")
        check_block(ctx, 0, 0, bits, a0, na, 0, bits, b0, nb, 17, 116, "overlay")
    truth = LDTruth(bits, 0, L, 17, 116)
    for genotype in (False, True):
        lo, hi = ld.windows_by_count(L, 0, L, 40)
        check_scores(ctx, 0, 0, truth, 0, L, lo, hi, 17, 116, genotype, "overlay")
    ctx.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_ld_refusals(gpu_lib):
    n, L = 50, 300
    cfg = SyntheticConfig(n, L, nchr=2, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, n_cv=10, seed=2, with_mutation=False)
    lo, hi = ld.windows_by_count(L, 0, L, 5)

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
    assert refused(lambda: ctx.ld_counts(0, 0), "no resident genotype planes") == -2
    assert refused(lambda: ctx.ld_scores(0, 0, lo, hi), "no resident genotype planes") == -2
    ctx.close()

    ctx = context(mine=(0,))
    assert refused(lambda: ctx.ld_counts(0, 1, 0, 10, 1, 0, 10), "not active") == -2
    assert refused(lambda: ctx.ld_counts(0, 0, 0, 10, 1, 0, 10), "not active") == -2
    assert refused(lambda: ctx.ld_scores(0, 1, lo[:10], hi[:10], 0, 10), "not active") == -2
    bits = unpacked(ctx, 0, 0)
    check_block(ctx, 0, 0, bits, 0, L, 0, bits, 0, L, 0, n, "one active chromosome")
    ctx.close()

    ctx = context(gen0=False)
    assert refused(lambda: ctx.ld_counts(0, 0, 0, L, 1, 0, L, 0, n), "no current generation") == -2
    assert refused(lambda: ctx.ld_scores(0, 0, lo, hi, 0, L, 0, n), "no current generation") == -2
    ctx.init_gen0(0, n, 77)
    rows = [unpacked(ctx, 0, c) for c in range(2)]
    truth = LDTruth(rows[0], 0, L, 0, n)

    def still_usable():
        check_block(ctx, 0, 0, rows[0], 3, 100, 1, rows[1], 150, 150, 0, n, "after a refusal")
        check_scores(ctx, 0, 0, truth, 0, L, lo, hi, 0, n, False, "after a refusal")
    still_usable()
    assert refused(lambda: ctx.ld_counts(0, 0, L - 1, 2), "SNPs (a)") == -1
    assert refused(lambda: ctx.ld_counts(0, 0, 0, L, 1, L + 1, 0), "SNPs (b)") == -1
    assert refused(lambda: ctx.ld_counts(0, 0, 0, L, 1, 0, L, n - 1, 2), "individuals") == -1
    assert refused(lambda: ctx.ld_scores(0, 0, lo[:2], hi[:2], L - 1, 2), "SNPs") == -1
    assert refused(lambda: ctx.ld_scores(0, 0, lo, hi, 0, L, n, 1), "individuals") == -1
    still_usable()
    for a, b in ((lo + 6, hi), (lo, hi - 6), (lo, hi + L), (lo[::-1].copy(), hi), (lo, np.where(np.arange(L) == 100, hi - 2, hi))):
        assert refused(lambda: ctx.ld_scores(0, 0, a, b), "window") == -1
    f = ctx.L._f("ld_scores")
    score = np.zeros(L, dtype=np.uint64)
    assert f(ctx.h, 0, 0, 0, L, lo, None, 0, n, 0, score, None) == -1 and "null window" in ctx.L.last_error()
    still_usable()
    ctx.close()
