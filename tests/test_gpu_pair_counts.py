"""gev_pair_genotype_counts / gev_ind_genotype_counts: per pair of individuals the loci where both are heterozygous, the loci where they
are opposite homozygotes and the genotype dot product, per individual the heterozygous and homozygous-alt loci and a weighted genotype
sum -- taken on the device from the resident rows (geneevolve_amd/csrc/gev_paircount.h: staged rows, one pass to bit planes, two exact
int8 matrix-core products).  The truth is numpy over gev_download_haps (x @ x.T, y @ z.T + z @ y.T, g @ g.T in int64), the route that
is pinned on the reference's own .hap files; every comparison is exact."""
import os

import numpy as np
import pytest

from geneevolve_amd import capi, relatedness
from geneevolve_amd.host import Simulation, SyntheticConfig
from tests import helpers
from tests.pair_counts_inputs import PairTruth, numpy_pair_counts, tile_mode
from tests.snp_counts_inputs import random_rows
from tests.test_gpu_snp_counts import overlay_situations, unpacked

pytestmark = pytest.mark.gpu

# (n_a, n_b), a_begin != b_begin: a swapped row / column map cannot pass the rectangular ones
BLOCKS = [(1, 1, 5, 200), (15, 17, 3, 100), (16, 16, 40, 7), (33, 129, 290, 11), (129, 33, 0, 300)]


def check_block(ctx, pop, chr, truth, s0, ns, a0, na, b0, nb, what):
    got = ctx.pair_genotype_counts(pop, chr, s0, ns, a0, na, b0, nb)
    want = truth.block(a0, na, b0, nb)
    label = f"{what}: SNPs [{s0},{s0 + ns}) a [{a0},+{na}) b [{b0},+{nb})"
    for name, g, w in zip(("n_hethet", "n_opphom", "dot"), got, want):
        assert g.dtype == np.uint32 and g.shape == (na, nb), label
        assert np.array_equal(g, w), f"{label}: {name} differs at {np.argwhere(g != w)[:5].tolist()}"
    return got


def check_ind(ctx, pop, chr, truth, s0, ns, i0, n, what):
    het, hom = ctx.ind_genotype_counts(pop, chr, s0, ns, i0, n)
    assert het.dtype == hom.dtype == np.uint32
    assert np.array_equal(het, truth.het[i0:i0 + n]) and np.array_equal(hom, truth.hom[i0:i0 + n]), f"{what}: SNPs [{s0},{s0 + ns}) individuals [{i0},+{n})"
    return het, hom


# ---- shapes that can go wrong ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[None, 4], ids=["default segments", "64-byte segments"])
def awkward(request, gpu_lib):
    """the 333 x 5000 population of test_counts_at_awkward_shapes (hot map, mutations, three generations), its rows and the truth of
    every SNP range the tests use"""
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
    bits = unpacked(ctx, 0, 0)
    # one SNP at both ends, across a word edge, across 64-locus edges from the last bit of a word to the first of another, whole
    snps = [(0, 1), (L - 1, 1), (31, 2), (63, 4097 - 63), (127, 130), (0, L)]
    truths = {r: PairTruth(bits, *r) for r in snps}
    yield ctx, n, L, snps, truths
    ctx.close()


def rectangular_blocks(awkward, what):
    ctx, n, L, snps, truths = awkward
    for s0, ns in snps:
        for na, nb, a0, b0 in BLOCKS:
            check_block(ctx, 0, 0, truths[(s0, ns)], s0, ns, a0, na, b0, nb, what)


def test_rectangular_blocks(awkward):
    rectangular_blocks(awkward, "awkward shapes")


def test_rectangular_blocks_on_the_large_tiles(awkward):
    """the same blocks and SNP ranges with the 128 x 128 instantiation forced (gev_dbg_bitprod_tiles(2)), which the compute-unit rule
    gives no block below about 2000 a side: one partly filled tile, down to one pair in it"""
    with tile_mode(awkward[0], 2) as t:
        rectangular_blocks(awkward, "awkward shapes, large tiles")
        assert t.launched() == (0, len(awkward[3]) * len(BLOCKS))


def whole_matrix_and_its_diagonal(awkward):
    ctx, n, L, snps, truths = awkward
    for s0, ns in ((0, L), (63, 4097 - 63)):
        t = truths[(s0, ns)]
        hethet, opphom, dot = check_block(ctx, 0, 0, t, s0, ns, 0, n, 0, n, "whole matrix")
        het, hom = check_ind(ctx, 0, 0, t, s0, ns, 0, n, "whole population")
        assert np.array_equal(np.diag(hethet), het) and not np.diag(opphom).any() and np.array_equal(np.diag(dot), het + 4 * hom)
        assert np.array_equal(hethet, hethet.T) and np.array_equal(dot, dot.T)
    check_ind(ctx, 0, 0, truths[(31, 2)], 31, 2, 17, 300, "a range of individuals")


def test_whole_matrix_and_its_diagonal(awkward):
    """333 x 333: three tiles a side, the last one partly filled.  The diagonal of a self block is the per-individual counts:
    n_hethet = n_het, n_opphom = 0, dot = n_het + 4 n_hom_alt"""
    whole_matrix_and_its_diagonal(awkward)


def test_whole_matrix_and_its_diagonal_on_the_large_tiles(awkward):
    """333 x 333 on tiles of 128 x 128: three tiles a side, the last one filled to 77"""
    with tile_mode(awkward[0], 2) as t:
        whole_matrix_and_its_diagonal(awkward)
        assert t.launched() == (0, 2)


def output_chunk_makes_no_difference(awkward):
    ctx, n, L, snps, truths = awkward
    ctx.dbg_output_chunk(7)
    try:
        for s0, ns in ((0, L), (127, 130)):
            for na, nb, a0, b0 in BLOCKS:
                check_block(ctx, 0, 0, truths[(s0, ns)], s0, ns, a0, na, b0, nb, "output chunk 7")
            check_ind(ctx, 0, 0, truths[(s0, ns)], s0, ns, 1, n - 2, "output chunk 7")
        check_block(ctx, 0, 0, truths[(0, L)], 0, L, 0, n, 0, n, "output chunk 7, whole matrix")
    finally:
        ctx.dbg_output_chunk(0)


def test_output_chunk_makes_no_difference(awkward):
    """gev_dbg_output_chunk(7): sub-blocks of 7 x 7 pairs, each staged, multiplied and copied out on its own"""
    output_chunk_makes_no_difference(awkward)


def test_output_chunk_makes_no_difference_on_the_large_tiles(awkward):
    """... each of them 7 x 7 pairs in the corner of one tile of 128 x 128"""
    with tile_mode(awkward[0], 2) as t:
        output_chunk_makes_no_difference(awkward)
        assert t.large_only()


def test_each_output_may_be_null_and_empty_requests(awkward):
    ctx, n, L, snps, truths = awkward
    f = ctx.L._f("pair_genotype_counts")
    want = truths[(0, L)].block(2, 20, 50, 30)
    for k in range(3):
        out = [None, None, None]
        out[k] = np.full((20, 30), 7, dtype=np.uint32)
        assert f(ctx.h, 0, 0, 0, L, 2, 20, 50, 30, out[0], out[1], out[2]) == 0
        assert np.array_equal(out[k], want[k])
    # n_snps == 0 writes zeros; n_a == 0 or n_b == 0 touches nothing
    m = [np.full((20, 30), 7, dtype=np.uint32) for _ in range(3)]
    assert f(ctx.h, 0, 0, 100, 0, 2, 20, 50, 30, m[0], m[1], m[2]) == 0
    assert not any(a.any() for a in m)
    m[0][:] = 7
    assert f(ctx.h, 0, 0, 0, L, 2, 0, 50, 30, m[0], None, None) == 0
    assert f(ctx.h, 0, 0, 0, L, 2, 20, n, 0, m[0], None, None) == 0
    assert (m[0] == 7).all()
    het, hom = ctx.ind_genotype_counts(0, 0, 100, 0, 5, 9)
    assert len(het) == 9 and not het.any() and not hom.any()
    assert len(ctx.ind_genotype_counts(0, 0, 0, L, n, 0)[0]) == 0


def test_weighted_sums_need_64_bits(awkward):
    ctx, n, L, snps, truths = awkward
    rs = np.random.RandomState(3)
    bits = unpacked(ctx, 0, 0)
    g = bits[0::2].astype(object) + bits[1::2].astype(object)
    for s0, ns in ((0, L), (63, 4097 - 63), (L - 1, 1)):
        w = rs.randint(0, 1 << 32, size=ns, dtype=np.uint64).astype(np.uint32)
        w[0] = w[-1] = 0xFFFFFFFF
        for i0, cnt in ((0, n), (7, 100)):
            het, hom, ws = ctx.ind_genotype_counts(0, 0, s0, ns, i0, cnt, weight=w)
            want = g[i0:i0 + cnt, s0:s0 + ns] @ w.astype(object)
            assert ws.dtype == np.uint64 and [int(v) for v in ws] == [int(v) for v in want], (s0, ns, i0, cnt)
            assert np.array_equal(het, truths[(s0, ns)].het[i0:i0 + cnt]) and np.array_equal(hom, truths[(s0, ns)].hom[i0:i0 + cnt])
            if ns == L:
                assert max(int(v) for v in ws) > 1 << 32
    ctx.dbg_output_chunk(7)
    try:
        w = np.full(L, 0xFFFFFFFF, dtype=np.uint32)
        ws = ctx.ind_genotype_counts(0, 0, 0, L, 0, n, weight=w)[2]
        assert [int(v) for v in ws] == [int(v) * 0xFFFFFFFF for v in g.sum(axis=1)]
    finally:
        ctx.dbg_output_chunk(0)


def check_block_by_matrix(ctx, bits, s0, ns, a0, na, b0, nb, what):
    """a block of thousands a side: one matrix of the truth at a time (products in float64: exact while 4 n_snps < 2^53), each dropped
    with its result once compared -> the largest entry of each matrix"""
    got = list(ctx.pair_genotype_counts(0, 0, s0, ns, a0, na, b0, nb))
    label = f"{what}: SNPs [{s0},{s0 + ns}) a [{a0},+{na}) b [{b0},+{nb})"
    largest = []
    for o, name in enumerate(("n_hethet", "n_opphom", "dot")):
        want = numpy_pair_counts(bits, s0, ns, a0, na, b0, nb, products=np.float64, only=o)
        assert got[o].dtype == np.uint32 and got[o].shape == (na, nb), label
        assert np.array_equal(got[o], want), f"{label}: {name} differs at {np.argwhere(got[o] != want)[:5].tolist()}"
        largest.append(int(got[o].max()))
        got[o] = want = None
    return largest


def test_blocks_wide_enough_for_the_large_tiles(gpu_lib):
    """The product takes tiles of 128 x 128 pairs where they give every compute unit work, of 64 x 64 otherwise; with the 256 compute
    units of an MI355X a block of 2100 x 2100 individuals (17 x 17 large tiles, the last one partly filled on both sides) and one of
    2200 x 2049 (18 x 17) launch on the large ones alone, which the launch counters of gev_dbg_bitprod_tiles assert; the 2100 x 2100
    block once more with the small tiles forced is a grid of 33 x 33 of them.  Then the walk at its real side, byte budgets alone:
    individuals (3, 4197) x (0, 4200) are one sub-block of 4096 x 4096 (32 x 32 large tiles) and, in the same call, the ragged
    remainders 4096 x 104, 101 x 4096 and 101 x 104 on 32, 32 and 1 small tiles, copied out at a pitch of 4200 with the count vectors
    of side B at offset 4096.  4200 individuals x 200 SNPs, founders with every allele frequency from 0 to 1; every sum is at most
    800, so the truth's products are exact in float64"""
    n, L = 4200, 200
    cfg = SyntheticConfig(n, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.05, n_cv=10, seed=6, with_mutation=False)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.upload_founders(0, 0, capi.pack_rows(random_rows(np.random.RandomState(23), n, L)), L)
    ctx.synth_cv_founders(0, 0, 0, 2 * n, 9)
    sim = Simulation(ctx, 79, 1, True)
    sim.ras_initial_human_gen0(0, n)
    sim.next_generation_rm(0, n)
    bits = unpacked(ctx, 0, 0)
    with tile_mode(ctx, 0) as t:
        hethet, opphom, dot = check_block_by_matrix(ctx, bits, 0, L, 0, 2100, 150, 2100, "2100 x 2100 individuals")
        assert hethet > 0 and opphom > 0 and dot > 255
        assert t.launched() == (0, 1), "17 x 17 large tiles are more than the compute units: the large tiles, and nothing else"
        check_block_by_matrix(ctx, bits, 1, 130, 3, 2200, 1, 2049, "2200 x 2049 individuals")
        assert t.launched() == (0, 1)
        check_block_by_matrix(ctx, bits, 1, 130, 3, 4197, 0, 4200, "4197 x 4200 individuals, sub-blocks of 4096")
        assert t.launched() == (3, 1), "one sub-block of 32 x 32 large tiles, three remainders on small ones"
    with tile_mode(ctx, 1) as t:
        check_block_by_matrix(ctx, bits, 0, L, 0, 2100, 150, 2100, "2100 x 2100 individuals, small tiles")
        assert t.launched() == (1, 0)
    ctx.close()


def test_sums_beyond_16_bits(gpu_lib):
    """64 individuals x 300 000 SNPs of allele frequency 0.5 at distinct positions, generation 0: the counts of a pair are near 75 000
    (both heterozygous) and 300 000 (dot), where no other pair test has a sum above 20 000 -- an accumulator or an output narrower than
    32 bits, or a count added in 16-bit halves, cannot pass.  Counts add over SNP ranges: the truth is summed over chunks of 50 000
    (products in float64: a chunk's sums are at most 200 000, exact)"""
    n, L = 64, 300_000
    cfg = SyntheticConfig(n, L, chrom_bp=3_000_000, map_step=20_000, rec_per_row=0.05, n_cv=10, seed=6, with_mutation=False)
    assert len(set(cfg.snp_pos.tolist())) == L
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.upload_founders(0, 0, capi.pack_rows(np.random.RandomState(24).randint(0, 2, size=(2 * n, L)).astype(np.uint8)), L)
    ctx.synth_cv_founders(0, 0, 0, 2 * n, 9)
    ctx.init_gen0(0, n, 80)
    bits = unpacked(ctx, 0, 0)
    want = [sum(m) for m in zip(*(numpy_pair_counts(bits, s0, min(50_000, L - s0), products=np.float64) for s0 in range(0, L, 50_000)))]
    got = ctx.pair_genotype_counts(0, 0)
    for name, g, w in zip(("n_hethet", "n_opphom", "dot"), got, want):
        assert g.dtype == np.uint32 and np.array_equal(g, w), f"{name} differs at {np.argwhere(g != w)[:5].tolist()}"
    assert int(got[0].max()) > 65535 and int(got[2].max()) > 65535 and int(np.min(got[2])) > 65535
    het, hom = ctx.ind_genotype_counts(0, 0)
    assert np.array_equal(het, np.diag(got[0])) and np.array_equal(het + 4 * hom, np.diag(got[2])) and int(het.min()) > 65535
    # a range that begins and ends inside a word
    s0, ns = 33, L - 70
    want = [sum(m) for m in zip(*(numpy_pair_counts(bits, a, min(50_000, s0 + ns - a), 1, 33, 0, n, products=np.float64) for a in range(s0, s0 + ns, 50_000)))]
    for name, g, w in zip(("n_hethet", "n_opphom", "dot"), ctx.pair_genotype_counts(0, 0, s0, ns, 1, 33, 0, n), want):
        assert np.array_equal(g, w), f"SNPs [{s0},+{ns}): {name} differs at {np.argwhere(g != w)[:5].tolist()}"
    ctx.close()


def test_the_tile_mode_hook(gpu_lib):
    """gev_dbg_bitprod_tiles: modes 0, 1, 2 and -1 (unchanged), GEV_EINVAL for any other, counters from the context's creation on,
    refused while a generation is pending"""
    n, L = 50, 300
    cfg = SyntheticConfig(n, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, n_cv=10, seed=2, with_mutation=False)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 50); ctx.synth_cv_founders(0, 0, 0, 2 * n, 60)
    sim = Simulation(ctx, 5, 1, True)
    sim.ras_initial_human_gen0(0, n)
    t = PairTruth(unpacked(ctx, 0, 0))
    assert ctx.dbg_bitprod_tiles() == (0, 0)
    ctx.L._f("dbg_bitprod_tiles")(ctx.h, -1, None)               # the counters may be left out
    check_block(ctx, 0, 0, t, 0, L, 0, n, 0, n, "tiles by compute units")
    assert ctx.dbg_bitprod_tiles() == (1, 0), "one tile: fewer than the compute units"
    assert ctx.dbg_bitprod_tiles(2) == (1, 0)
    check_block(ctx, 0, 0, t, 0, L, 0, n, 0, n, "large tiles")
    assert ctx.dbg_bitprod_tiles(-1) == (1, 1)
    check_block(ctx, 0, 0, t, 0, L, 0, n, 0, n, "large tiles still")
    for mode in (3, -2, 128):
        with pytest.raises(capi.GevError) as e:
            ctx.dbg_bitprod_tiles(mode)
        assert e.value.code == -1 and "mode" in str(e.value)
    check_block(ctx, 0, 0, t, 0, L, 0, n, 0, n, "large tiles after a refusal")
    assert ctx.dbg_bitprod_tiles(1) == (1, 3)
    check_block(ctx, 0, 0, t, 0, L, 0, n, 0, n, "small tiles")
    assert ctx.dbg_bitprod_tiles(0) == (2, 3)
    ctx.generation_begin(0, sim.glob.x, n)
    with pytest.raises(capi.GevError) as e:
        ctx.dbg_bitprod_tiles(2)
    assert e.value.code == -2 and "pending" in str(e.value)
    ctx.generation_end()
    assert ctx.dbg_bitprod_tiles() == (2, 3)
    ctx.close()


# ---- fixture replays -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dense", "ex1mut", "mig2"])
def test_pair_counts_of_replayed_fixtures(gpu_lib, oracle_lib, case):
    """the fixture's generations replayed through the library (recorded couples, seeds and moves; ex1mut: mutation map and three
    chromosomes; mig2: the last step is a migration, so the logical row order differs from the physical one and the pair count is the
    first call to ask for it).  At the last generation, for every population and chromosome: the whole matrix, a rectangular block over
    a sub-range of SNPs, the per-individual counts; over all chromosomes: relatedness.pair_counts and the statistics made of it."""
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
        first = ctx.pair_genotype_counts(ip, 0)                       # before anything else has asked for the population's rows
        per_chr = []
        for ic in range(nchr):
            L = ctx._nsnp[(ip, ic)]
            bits = unpacked(ctx, ip, ic)
            t = PairTruth(bits)
            per_chr.append(t)
            if ic == 0:
                for g, w in zip(first, (t.hethet, t.opphom, t.dot)):
                    assert np.array_equal(g, w), f"{case}: population {ip}, the first call"
            check_block(ctx, ip, ic, t, 0, L, 0, n, 0, n, f"{case} population {ip} chromosome {ic}")
            check_ind(ctx, ip, ic, t, 0, L, 0, n, f"{case} population {ip} chromosome {ic}")
            s0, ns = L // 3, L // 3 + 1
            a0, na, b0, nb = 1, n // 2, n // 3, n - n // 3
            sub = PairTruth(bits, s0, ns)
            check_block(ctx, ip, ic, sub, s0, ns, a0, na, b0, nb, f"{case} population {ip} chromosome {ic}")
            check_ind(ctx, ip, ic, sub, s0, ns, n // 3, n - n // 3, f"{case} population {ip} chromosome {ic}")
        # summed over the chromosomes
        a, b = (1, n - 2), (0, n // 2 + 1)
        pc = relatedness.pair_counts(ctx, ip, a, b)
        ra, rb = slice(a[0], a[0] + a[1]), slice(b[0], b[0] + b[1])
        assert pc.n_snps == sum(ctx._nsnp[(ip, ic)] for ic in range(nchr))
        for name in ("hethet", "opphom", "dot"):
            assert np.array_equal(getattr(pc, "n_" + name if name != "dot" else name), sum(getattr(t, name)[ra, rb] for t in per_chr)), name
        assert np.array_equal(pc.het_a, sum(t.het[ra].astype(np.int64) for t in per_chr)) and np.array_equal(pc.hom_b, sum(t.hom[rb].astype(np.int64) for t in per_chr))
        g = np.concatenate([unpacked(ctx, ip, ic)[0::2].astype(np.int64) + unpacked(ctx, ip, ic)[1::2] for ic in range(nchr)], axis=1)
        assert np.array_equal(relatedness.ibs_distance(pc), np.abs(g[ra, None, :] - g[None, rb, :]).sum(axis=2))
        whole = relatedness.pair_counts(ctx, ip)
        assert np.array_equal(np.diag(relatedness.king_kinship(whole)), np.full(n, 0.5))
        grm = relatedness.grm_vanraden(ctx, ip, a, b)
        p = g.sum(axis=0) / (2.0 * n)
        zc = g - 2.0 * p
        assert np.allclose(grm, (zc[ra] @ zc[rb].T) / (2.0 * p * (1.0 - p)).sum(), rtol=1e-9, atol=1e-9)
    if case == "ex1mut":
        assert nchr == 3
    ctx.close()


# ---- mutation overlay ------------------------------------------------------------------------------------------------------------------
def test_pair_counts_under_the_mutation_overlay(gpu_lib):
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
    for s0, ns in ((0, L), (10, 3), (11, 1), (301, 350), (129, 571)):
        t = PairTruth(bits, s0, ns)
        check_block(ctx, 0, 0, t, s0, ns, 0, n, 0, n, "overlay")
        check_block(ctx, 0, 0, t, s0, ns, 17, 116, 0, 1, "overlay")
        check_ind(ctx, 0, 0, t, s0, ns, 0, n, "overlay")
    ctx.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_pair_counts_refusals(gpu_lib):
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
    assert refused(lambda: ctx.pair_genotype_counts(0, 0), "no resident genotype planes") == -2
    assert refused(lambda: ctx.ind_genotype_counts(0, 0), "no resident genotype planes") == -2
    ctx.close()

    ctx = context(mine=(0,))
    assert ctx.active_chrs() == [0]
    assert refused(lambda: ctx.pair_genotype_counts(0, 1, 0, 10), "not active") == -2
    assert refused(lambda: ctx.ind_genotype_counts(0, 1, 0, 10), "not active") == -2
    t = PairTruth(unpacked(ctx, 0, 0))
    check_block(ctx, 0, 0, t, 0, L, 0, n, 0, n, "one active chromosome")
    pc = relatedness.pair_counts(ctx, 0)                              # skips the inactive chromosome
    assert pc.n_snps == L and np.array_equal(pc.dot, t.dot)
    ctx.close()

    ctx = context(gen0=False)
    assert refused(lambda: ctx.pair_genotype_counts(0, 0, 0, L, 0, n, 0, n), "no current generation") == -2
    assert refused(lambda: ctx.ind_genotype_counts(0, 0, 0, L, 0, n), "no current generation") == -2
    ctx.init_gen0(0, n, 77)
    t = PairTruth(unpacked(ctx, 0, 0))

    def still_usable():
        check_block(ctx, 0, 0, t, 0, L, 0, n, 0, n, "after a refusal")
    still_usable()
    assert refused(lambda: ctx.pair_genotype_counts(0, 0, L - 1, 2), "SNPs") == -1
    assert refused(lambda: ctx.pair_genotype_counts(0, 0, L + 1, 0), "SNPs") == -1
    assert refused(lambda: ctx.pair_genotype_counts(0, 0, 0, L, n - 1, 2, 0, n), "individuals (a)") == -1
    assert refused(lambda: ctx.pair_genotype_counts(0, 0, 0, L, 0, n, n - 1, 2), "individuals (b)") == -1
    assert refused(lambda: ctx.pair_genotype_counts(0, 0, 0, L, 0, n, n + 1, 0), "individuals (b)") == -1
    assert refused(lambda: ctx.ind_genotype_counts(0, 0, L - 1, 2), "SNPs") == -1
    assert refused(lambda: ctx.ind_genotype_counts(0, 0, 0, L, n - 1, 2), "individuals") == -1
    still_usable()
    # weights and wsum come together
    f = ctx.L._f("ind_genotype_counts")
    w = np.ones(L, dtype=np.uint32); ws = np.zeros(n, dtype=np.uint64)
    assert f(ctx.h, 0, 0, 0, L, 0, n, w, None, None, None) == -1 and "wsum" in ctx.L.last_error()
    assert f(ctx.h, 0, 0, 0, L, 0, n, None, None, None, ws) == -1 and "wsum" in ctx.L.last_error()
    assert f(ctx.h, 0, 0, 0, L, 0, n, w, None, None, ws) == 0
    assert np.array_equal(ws, t.het.astype(np.uint64) + 2 * t.hom.astype(np.uint64))
    still_usable()
    t1 = PairTruth(unpacked(ctx, 0, 1), 299, 1)
    check_block(ctx, 0, 1, t1, 299, 1, 49, 1, 0, n, "second chromosome")
    ctx.close()
