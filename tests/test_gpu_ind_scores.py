"""gev_ind_scores: per individual and weight column the sum of the column's weights times the genotype and over the heterozygous SNPs --
taken on the device from the current generation (geneevolve_amd/csrc/gev_indscore.h: the two planes of the pair calls against the
weights' digits laid out in the planes' byte order, exact int8 matrix-core products, the SNPs split over workgroups).  The truth is
numpy over gev_download_haps (tests/ind_scores_inputs.py); the host build of the same arithmetic is held against it too.  Then
scores.py and pca.py on the device's integers.  Every comparison is exact."""
import os

import numpy as np
import pytest

from geneevolve_amd import capi, pca, scores
from geneevolve_amd.host import Simulation, SyntheticConfig
from tests import helpers
from tests.ind_scores_inputs import L, N_PEOPLE, NAMES, STEP, W_MAX, genotypes, numpy_scores, one_hot_value, one_hot_weights, population_rows, random_weights
from tests.test_gpu_snp_counts import overlay_situations, unpacked
from tests.test_gpu_trait_sums import founder_plane
from tests.trait_sums_inputs import NAMES as TS_NAMES, numpy_trait_sums, random_quanta

pytestmark = pytest.mark.gpu

# individuals: everybody, from inside a fragment of 16 across fragments, one tile of 128 on no tile edge, one, the last ones
IND = [(0, N_PEOPLE), (5, 129), (3, 128), (100, 1), (133, 17)]
# SNPs: everything (three slices of 4096), inside a word, the last one, across the slice edge, a step on a step, across words, across a step
SNPS = [(0, L), (56, 15), (L - 1, 1), (4033, 64 + 63), (4096, 256), (63, 65), (130, 257)]
N_SCORES = (1, 4, 5, 17)


def check(ctx, pop, chr, geno, w, s0, ns, i0, ni, what, rows=None, row_L=None):
    """the device against numpy and, with the packed rows, against the host build"""
    got = ctx.ind_scores(pop, chr, w, s0, ns, i0, ni)
    want = numpy_scores(geno, s0, ns, i0, ni, w)
    label = f"{what}: chr {chr} SNPs [{s0},+{ns}) individuals [{i0},+{ni}) {np.atleast_2d(w).shape[0]} columns"
    for name, g, x in zip(NAMES, got, want):
        assert g.dtype == np.int64 and g.shape == x.shape, f"{label}: {name}"
        assert np.array_equal(g, x), f"{label}: {name} differs at {np.argwhere(g != x)[:5].tolist()}"
    if rows is not None:
        host = ctx.L.dbg_ind_scores_host(rows, geno.shape[1] if row_L is None else row_L, w, s0, ns, i0, ni)
        assert all(np.array_equal(g, h) for g, h in zip(got, host)), f"{label}: device and host build differ"
    return got


@pytest.fixture(scope="module", params=[None, 4], ids=["default segments", "64-byte segments"])
def founders(request, gpu_lib):
    """the 150 x 8269 rows of the CPU test as the founders of generation 0 (no breeding: the rows of the planes are the uploaded ones, in
    the order generation 0 drew them): the context, the 0/1/2 matrix and the packed rows as gev_download_haps returns them"""
    seg_chunks = request.param
    old = os.environ.get("GEV_SEG_CHUNKS")
    if seg_chunks:
        os.environ["GEV_SEG_CHUNKS"] = str(seg_chunks)
    try:
        cfg = SyntheticConfig(N_PEOPLE, L, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.05, n_cv=20, seed=5, with_mutation=False)
        ctx = gpu_lib.create(1, 1, 1)
        cfg.apply_static(ctx)
        ctx.upload_founders(0, 0, capi.pack_rows(population_rows()), L)
        ctx.synth_cv_founders(0, 0, 0, 2 * N_PEOPLE, 32)
        Simulation(ctx, 4242, 1, True).ras_initial_human_gen0(0, N_PEOPLE)
        if seg_chunks:
            assert ctx.plane_ptr(0, 0)[1] == 64, "64-byte segments"
    finally:
        if seg_chunks:
            if old is None:
                del os.environ["GEV_SEG_CHUNKS"]
            else:
                os.environ["GEV_SEG_CHUNKS"] = old
    rows = ctx.download_haps(0, 0)
    geno = genotypes(capi.unpack_rows(rows, L))
    yield ctx, geno, rows
    ctx.close()


@pytest.mark.parametrize("first", [0, 3, 64, 100, 4096, L - STEP], ids=lambda b: f"first SNP {b}")
def test_one_hot_columns_tell_the_byte_order(founders, first):
    """for every byte position p of a step a column whose only weight sits at SNP first + p, a different value with four non-zero digits
    at each: gscore[p][i] = g_ip w_p, so one misplaced byte of the weight operand is one wrong entry.  From the first SNP of a word, of
    a step and of a slice, from inside a word, and at the row's end; in a range that begins with them and in one that begins before
    them, inside a word.  64 column groups: the grid's z"""
    ctx, geno, rows = founders
    vals = np.array([one_hot_value(p) for p in range(STEP)], dtype=np.int64)
    for s0 in sorted({first, max(first - 37, 0)}):
        ns = min(first + STEP + 70, L) - s0
        gscore, hetscore = check(ctx, 0, 0, geno, one_hot_weights(ns, first - s0), s0, ns, 0, N_PEOPLE, f"one-hot from {first}", rows)
        g = geno[:, first:first + STEP].T
        assert np.array_equal(gscore, g * vals[:, None]) and np.array_equal(hetscore, (g == 1) * vals[:, None])


@pytest.mark.parametrize("chunk", [0, 7], ids=["byte budgets", "output chunk 7"])
def test_ranges_of_individuals_and_snps(founders, chunk):
    """every range of individuals against every range of SNPs with 1, 4, 5 and 17 columns in turn; with gev_dbg_output_chunk(7) a block
    is 7 individuals staged in passes of 3, so everybody is 22 blocks whose scores land side by side in the caller's matrices"""
    ctx, geno, rows = founders
    rs = np.random.RandomState(60 + chunk)
    ctx.dbg_output_chunk(chunk)
    try:
        k = 0
        for i0, ni in IND:
            for s0, ns in SNPS:
                check(ctx, 0, 0, geno, random_weights(rs, N_SCORES[k % 4], ns), s0, ns, i0, ni, f"chunk {chunk}", rows); k += 1
    finally:
        ctx.dbg_output_chunk(0)


@pytest.mark.parametrize("n_scores", N_SCORES)
def test_every_number_of_columns_on_everybody(founders, n_scores):
    ctx, geno, rows = founders
    w = random_weights(np.random.RandomState(n_scores), n_scores, L)
    first = check(ctx, 0, 0, geno, w, 0, L, 0, N_PEOPLE, "everybody", rows)
    again = ctx.ind_scores(0, 0, w, 0, L, 0, N_PEOPLE)
    assert all(np.array_equal(a, b) for a, b in zip(first, again)), "a repeat of the call gives the same integers"
    if n_scores == 1:
        check(ctx, 0, 0, geno, w[0], 0, L, 0, N_PEOPLE, "one column as a vector")


def test_every_weight_at_the_bound(founders):
    """every weight +-2^30 over the whole row: every digit sum as large as 8269 SNPs make it; one column all +2^30"""
    ctx, geno, rows = founders
    rs = np.random.RandomState(5)
    extreme = np.where(rs.random_sample((2, L)) < 0.5, W_MAX, -W_MAX).astype(np.int32); extreme[1] = W_MAX
    gscore = check(ctx, 0, 0, geno, extreme, 0, L, 0, N_PEOPLE, "weights at +-2^30", rows)[0]
    assert np.array_equal(gscore[1], geno.sum(axis=1) << 30)


def test_against_the_counts_per_individual(founders):
    """one column of non-negative weights: gscore is the wsum of gev_ind_genotype_counts; a column of ones: gscore = n_het + 2 n_hom_alt
    and hetscore = n_het"""
    ctx, geno, rows = founders
    rs = np.random.RandomState(6)
    for (s0, ns), (i0, ni) in (((0, L), (0, N_PEOPLE)), ((130, 257), (5, 129)), ((4033, 127), (133, 17))):
        w = rs.randint(0, W_MAX + 1, size=ns).astype(np.uint32)
        het, hom, wsum = ctx.ind_genotype_counts(0, 0, s0, ns, i0, ni, weight=w)
        gscore, hetscore = ctx.ind_scores(0, 0, w.astype(np.int32), s0, ns, i0, ni)
        assert np.array_equal(gscore[0], wsum.astype(np.int64))
        gscore, hetscore = ctx.ind_scores(0, 0, np.ones(ns, dtype=np.int32), s0, ns, i0, ni)
        assert np.array_equal(gscore[0], het.astype(np.int64) + 2 * hom) and np.array_equal(hetscore[0], het)


def test_each_output_may_be_null_and_empty_requests(founders):
    ctx, geno, rows = founders
    f = ctx.L._f("ind_scores")
    w = random_weights(np.random.RandomState(2), 3, 200)
    want = numpy_scores(geno, 70, 200, 5, 20, w)
    for k in range(2):
        out = [None, None]
        out[k] = np.full((3, 20), 7, dtype=np.int64)
        assert f(ctx.h, 0, 0, 70, 200, 5, 20, w, 3, *out) == 0
        assert np.array_equal(out[k], want[k]), NAMES[k]
        only = ctx.ind_scores(0, 0, w, 70, 200, 5, 20, want=(k == 0, k == 1))
        assert only[1 - k] is None and np.array_equal(only[k], want[k])
    outs = [np.full((3, 20), 7, dtype=np.int64) for _ in range(2)]
    assert f(ctx.h, 0, 0, 70, 200, 5, 0, w, 3, *outs) == 0 and all((a == 7).all() for a in outs), "no individual: nothing is touched"
    assert f(ctx.h, 0, 0, 70, 0, 5, 20, None, 3, *outs) == 0 and not any(a.any() for a in outs), "no SNP: zeros"
    assert f(ctx.h, 0, 0, 70, 200, 5, 20, w, 3, None, None) == 0
    got = ctx.ind_scores(0, 0, np.zeros((0, 200), dtype=np.int32), 70, 200, 5, 20)
    assert got[0].shape == got[1].shape == (0, 20)


@pytest.mark.parametrize("chunk", [0, 7], ids=["byte budgets", "output chunk 7"])
def test_scores_and_trait_sums_take_turns_on_one_context(founders, chunk):
    """the two calls share one set of scratch buffers (gev_digitprod.h): scores and trait sums alternate on one context, so that the set
    is grown and reused across the two layouts -- 17 columns on everything, one on a few, then the other way round, a trait-sum call
    that wants the counts alone and so touches none of it, and the first call again.  Every result equals its host build and numpy"""
    ctx, geno, rows = founders
    bits = capi.unpack_rows(rows, L)
    rs = np.random.RandomState(70 + chunk)

    def trait_sums(q, s0, ns, i0, ni):
        got = ctx.snp_trait_sums(0, 0, q, s0, ns, i0, ni)
        host = ctx.L.dbg_trait_sums_host(rows, L, q, s0, ns, i0, ni)
        for name, g, h, x in zip(TS_NAMES, got, host, numpy_trait_sums(bits, s0, ns, i0, ni, q)):
            assert g.shape == x.shape and np.array_equal(g, x) and np.array_equal(g, h), f"chunk {chunk}: {name} of {q.shape[0]} traits, SNPs [{s0},+{ns}) individuals [{i0},+{ni})"

    ctx.dbg_output_chunk(chunk)
    try:
        w17 = random_weights(rs, 17, L)
        first = check(ctx, 0, 0, geno, w17, 0, L, 0, N_PEOPLE, f"chunk {chunk}, first", rows)
        trait_sums(random_quanta(rs, 1, 129), 63, 130, 5, 129)
        check(ctx, 0, 0, geno, random_weights(rs, 1, 15), 56, 15, 100, 1, f"chunk {chunk}, one column", rows)
        trait_sums(random_quanta(rs, 17, N_PEOPLE), 0, L, 0, N_PEOPLE)
        trait_sums(np.zeros((0, N_PEOPLE), dtype=np.int32), 0, L, 0, N_PEOPLE)
        again = check(ctx, 0, 0, geno, w17, 0, L, 0, N_PEOPLE, f"chunk {chunk}, again", rows)
        assert all(np.array_equal(a, b) for a, b in zip(first, again)), "the first call again gives the same integers"
    finally:
        ctx.dbg_output_chunk(0)


# ---- the mutation overlay and fixture replays ------------------------------------------------------------------------------------------
def test_scores_under_the_mutation_overlay(gpu_lib):
    """the population of test_counts_under_the_mutation_overlay: mutations on SNPs whose founder bit was 1, on both haplotypes of an
    individual, repeated within a list, at positions that several SNP columns share.  The overlay is at work: the scores differ from
    those of the rows without it"""
    n, Ls = 150, 700
    cfg = SyntheticConfig(n, Ls, chrom_bp=1400, map_step=100, rec_per_row=0.05, mut_per_row=0.2, n_cv=8, seed=4)
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
    geno = genotypes(bits)
    rs = np.random.RandomState(3)
    for s0, ns in ((0, Ls), (10, 3), (301, 350)):
        check(ctx, 0, 0, geno, random_weights(rs, 5, ns), s0, ns, 0, n, "overlay")
        check(ctx, 0, 0, geno, random_weights(rs, 4, ns), s0, ns, 17, 116, "overlay")
    ones = np.ones((1, Ls), dtype=np.int32)
    got = ctx.ind_scores(0, 0, ones)
    plain = numpy_scores(genotypes(founder_plane(ctx, 0, 0, bits, cfg.snp_pos)), 0, Ls, 0, n, ones)
    assert (got[0] != plain[0]).any() and (got[1] != plain[1]).any(), "scores that the mutation overlay changes"
    ctx.close()


def replayed(gpu_lib, oracle_lib, case):
    """the fixture's generations replayed through the library -> the context at the last generation"""
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
    return ctx, n_pop, nchr


def test_scores_of_the_replayed_dense_fixture(gpu_lib, oracle_lib):
    """dense: mutations lie on SNPs.  At the last generation, for every chromosome: the first call before anything else has asked for
    the population's rows, everybody and a sub-range, 5 columns"""
    ctx, n_pop, nchr = replayed(gpu_lib, oracle_lib, "dense")
    rs = np.random.RandomState(12)
    for ip in range(n_pop):
        n = ctx.pop_size(ip)
        first = ctx.ind_scores(ip, 0, np.ones(ctx._nsnp[(ip, 0)], dtype=np.int32))
        for ic in range(nchr):
            Lc = ctx._nsnp[(ip, ic)]
            rows = ctx.download_haps(ip, ic)
            geno = genotypes(capi.unpack_rows(rows, Lc))
            if ic == 0:
                assert np.array_equal(first[0][0], geno.sum(axis=1)), "the first call"
            check(ctx, ip, ic, geno, random_weights(rs, 5, Lc), 0, Lc, 0, n, "dense", rows)
            i0, ni = n // 4, n - n // 3
            ns = min(Lc, 300)
            check(ctx, ip, ic, geno, random_weights(rs, 5, ns), (Lc - ns) // 2, ns, i0, ni, "dense", rows)
    ctx.close()


def test_scores_summed_over_the_chromosomes_of_ex1mut(gpu_lib, oracle_lib):
    """scores.sums over the three chromosomes of ex1mut (mutation map), and over two of them; scores.prs within the quantisation"""
    ctx, n_pop, nchr = replayed(gpu_lib, oracle_lib, "ex1mut")
    assert nchr == 3
    rs = np.random.RandomState(13)
    n = ctx.pop_size(0)
    geno = {ic: genotypes(capi.unpack_rows(ctx.download_haps(0, ic), ctx._nsnp[(0, ic)])) for ic in range(nchr)}
    q = {ic: random_weights(rs, 6, geno[ic].shape[1]) for ic in range(nchr)}
    for chrs, ind in (((0, 1, 2), None), ((0, 2), (n // 5, n // 2))):
        i0, ni = (0, n) if ind is None else ind
        want = [sum(numpy_scores(geno[ic], 0, geno[ic].shape[1], i0, ni, q[ic])[k] for ic in chrs) for k in range(2)]
        got = scores.sums(ctx, 0, {ic: q[ic] for ic in chrs}, ind)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), chrs
    beta = {ic: rs.normal(0, 1, (2, geno[ic].shape[1])) for ic in range(nchr)}
    exact = sum(beta[ic] @ geno[ic].T.astype(np.float64) for ic in range(nchr))
    top = max(np.abs(beta[ic]).max() for ic in range(nchr))
    n_snps = sum(g.shape[1] for g in geno.values())
    assert (np.abs(scores.prs(ctx, 0, beta) - exact) <= 2 * n_snps * top / float(1 << 31) + 1e-12 * np.abs(exact).max()).all()
    ctx.close()


# ---- with the trait sums: the transpose identity and the principal components -----------------------------------------------------------
def test_transpose_identity_with_the_trait_sums(gpu_lib):
    """y^T (G w) = (G^T y)^T w: for random quanta Y and weights W on a bred 48 x 20 000 population, sum_i y[t][i] gscore[s][i] ==
    sum_j w[s][j] gsum[t][j] for every pair of a trait and a column, both sides formed in Python integers -- the two matrix-core
    products, made by different kernels from different planes, agree on every bit"""
    n, Lt = 48, 20000
    cfg = SyntheticConfig(n, Lt, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.05, mut_per_row=2e-3, n_cv=10, seed=9)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 3); ctx.synth_cv_founders(0, 0, 0, 2 * n, 4)
    sim = Simulation(ctx, 77, 1, True)
    sim.ras_initial_human_gen0(0, n)
    for _ in range(2):
        sim.next_generation_rm(0, n)
    rs = np.random.RandomState(10)
    y = random_weights(rs, 3, n); w = random_weights(rs, 5, Lt)
    gscore, hetscore = ctx.ind_scores(0, 0, w)
    gsum, hetsum, het, hom = ctx.snp_trait_sums(0, 0, y)
    for a, b in ((gscore, gsum), (hetscore, hetsum)):
        left = y.astype(object) @ a.astype(object).T                 # [traits][columns]
        right = b.astype(object) @ w.astype(object).T
        assert left.shape == (3, 5) and (left == right).all() and all(isinstance(v, int) for v in left.ravel())
        assert any(abs(v) >= 1 << 63 for v in left.ravel()), "sums that an int64 would not hold"
    ctx.close()


def test_components_from_the_device_equal_those_from_the_host_builds(gpu_lib):
    """pca.components on a context of two populations that share their SNPs, fed by the device's two products and by the host builds on
    the downloaded rows: the integer products are equal, so every float that follows is the same -- bit for bit; and pca.project"""
    n, Lp = (90, 70), 1500
    cfg = SyntheticConfig(n[0], Lp, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.05, mut_per_row=1e-3, n_cv=10, seed=12)
    ctx = gpu_lib.create(2, 1, 1)
    for ip in range(2):
        cfg.apply_static(ctx, ip)
        ctx.synth_founders(ip, 0, 2 * n[ip], 21 + ip); ctx.synth_cv_founders(ip, 0, 0, 2 * n[ip], 31 + ip)
    sim = Simulation(ctx, 5, 1, True)
    for ip in range(2):
        sim.ras_initial_human_gen0(ip, n[ip])
        sim.next_generation_rm(ip, n[ip])
    rows = [ctx.download_haps(ip, 0) for ip in range(2)]
    lib = ctx.L
    host = (lambda pop, chr, q: lib.dbg_ind_scores_host(rows[pop], Lp, q, want=(True, False))[0],
            lambda pop, chr, q: lib.dbg_trait_sums_host(rows[pop], Lp, q)[0])
    dev = pca.components(ctx, [0, 1], 3, iters=3)
    ref = pca.components(ctx, [0, 1], 3, iters=3, products=host)
    assert dev.n_snps == ref.n_snps > Lp // 2 and dev.vectors.shape == (sum(n), 3)
    assert np.array_equal(dev.values, ref.values) and np.array_equal(dev.vectors, ref.vectors) and np.array_equal(dev.ritz, ref.ritz)
    assert np.array_equal(dev.loadings_by_chr[0], ref.loadings_by_chr[0]) and np.array_equal(dev.offset, ref.offset)
    for ip in range(2):
        assert np.array_equal(pca.project(ctx, ip, dev.loadings_by_chr, dev.offset), pca.project(ctx, ip, ref.loadings_by_chr, ref.offset, products=host))
    ctx.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_ind_scores_refusals(gpu_lib):
    n, Lr = 50, 300
    cfg = SyntheticConfig(n, Lr, nchr=2, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, n_cv=10, seed=2, with_mutation=False)
    w = np.zeros((2, Lr), dtype=np.int32)

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
    assert refused(lambda: ctx.ind_scores(0, 0, w, 0, Lr, 0, n), "no resident genotype planes") == -2
    ctx.close()

    ctx = context(mine=(0,))
    assert refused(lambda: ctx.ind_scores(0, 1, w[:, :10], 0, 10, 0, n), "not active") == -2
    check(ctx, 0, 0, genotypes(unpacked(ctx, 0, 0)), w + 3, 0, Lr, 0, n, "one active chromosome")
    ctx.close()

    ctx = context(gen0=False)
    assert refused(lambda: ctx.ind_scores(0, 0, w, 0, Lr, 0, n), "no current generation") == -2
    ctx.init_gen0(0, n, 77)
    geno = genotypes(unpacked(ctx, 0, 1))
    rs = np.random.RandomState(1)

    def still_usable():
        check(ctx, 0, 1, geno, random_weights(rs, 5, 100), 3, 100, 7, 40, "after a refusal")
    still_usable()
    assert refused(lambda: ctx.ind_scores(0, 0, w[:, :2], Lr - 1, 2, 0, n), "SNPs") == -1
    assert refused(lambda: ctx.ind_scores(0, 0, w, 0, Lr, n - 1, 2), "individuals") == -1
    for bad in (W_MAX + 1, -W_MAX - 1):
        w1 = w.copy(); w1[1, Lr - 1] = bad
        assert refused(lambda: ctx.ind_scores(0, 0, w1, 0, Lr, 0, n), "weight") == -1
    f = ctx.L._f("ind_scores")
    out = np.zeros((2, n), dtype=np.int64)
    assert f(ctx.h, 0, 0, 0, Lr, 0, n, None, 2, out, None) == -1 and "null weight" in gpu_lib.last_error()
    still_usable()
    ctx.close()
    # more than 2^22 SNPs: refused before anything is touched (the chromosome itself is shorter, so the range is refused first there;
    # the bound is pinned on the host build, which takes the count of SNPs as an argument)
    big = (1 << 22) + 1
    fh = gpu_lib._f("dbg_ind_scores_host")
    assert fh(None, 0, 10, big, 0, big, 0, 1, None, 1, None, None) == -5 and "at most" in gpu_lib.last_error()
