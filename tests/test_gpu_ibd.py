"""gev_ibd_sharing / gev_ancestry_bp: identity by descent per pair of haplotype rows walked on the device from the ancestry interval
lists, against the per-position raster of tests/ibd_inputs.py on the lists gev_download_intervals returns and against the same header
built for the host: an inbred population (rows of 19 to 37 parts, pairs with up to 11 segments), thresholds, row ranges around the
16-row tile and the 8-row wave block, null outputs, a context without genotype planes, two populations behind
a migration, the refusals, and the reductions of geneevolve_amd/ibd.py (pytest -m gpu)."""
from fractions import Fraction

import numpy as np
import pytest

from geneevolve_amd import capi, ibd
from geneevolve_amd.host import Simulation, SyntheticConfig
from tests import ibd_inputs as T
from tests.synth import synth_packed

pytestmark = pytest.mark.gpu

N, GENS = 40, 12
NAMES = ("shared_bp", "n_seg", "max_seg")
RANGES = [(0, 80), (1, 1), (3, 17), (15, 33), (64, 16), (79, 1)]


def inbred_config():
    return SyntheticConfig(N, 64, nchr=1, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.02, mut_per_row=2e-3, n_cv=8, seed=5)


def build_inbred(lib, dense=True, upload=False):
    """the inbred population on a context of `lib` (upload: founders from the host, for a library without the device generator)"""
    cfg = inbred_config()
    ctx = lib.create(1, 1, 1)
    if not dense:
        ctx.set_dense_state(False)
    cfg.apply_static(ctx)
    if upload:
        ctx.upload_founders(0, 0, synth_packed(31, 2 * N, 64), 64); ctx.upload_cv_founders(0, 0, 0, synth_packed(32, 2 * N, 8), 8)
    else:
        if dense:
            ctx.synth_founders(0, 0, 2 * N, 31)
        ctx.synth_cv_founders(0, 0, 0, 2 * N, 32)
    sim = Simulation(ctx, 4242, 1, True)
    sim.ras_initial_human_gen0(0, N)
    for _ in range(GENS):
        sim.next_generation_rm(0, N)
    return ctx, sim


def fixture_conditions(parts, off, segs):
    """what the cases below need of the population, asserted from the truth -> the figures"""
    n = len(off) - 1
    per_row = np.diff(off.astype(np.int64))
    nseg = np.array([[len(segs[a][b]) for b in range(n)] for a in range(n)])
    off_diag = nseg[~np.eye(n, dtype=bool)]
    fig = {"rows": n, "parts_min": int(per_row.min()), "parts_max": int(per_row.max()), "none": float((off_diag == 0).mean()),
           "multi": float((off_diag >= 2).mean()), "most": int(off_diag.max()), "adjacent": T.adjacent_same_label(parts, off)}
    assert fig["none"] >= 0.01, fig
    assert fig["multi"] >= 0.5, fig
    assert fig["adjacent"] >= 1, fig
    return fig


class Inbred:
    def __init__(self, lib):
        self.lib = lib
        self.ctx, self.sim = build_inbred(lib)
        self.parts, self.off = self.ctx.download_intervals(0, 0)
        self.segs = T.all_segments(self.parts, self.off)
        self.figures = fixture_conditions(self.parts, self.off, self.segs)
        self.span = int(inbred_config().rmap_bp[-1] - inbred_config().rmap_bp[0])
        self._truth = {}

    def truth(self, min_bp=0):
        """the raster's three matrices over all rows (computed once per threshold and left unchanged)"""
        if min_bp not in self._truth:
            self._truth[min_bp] = T.truth(self.parts, self.off, min_bp=min_bp, seg_lists=self.segs)
            for m in self._truth[min_bp]:
                m.setflags(write=False)
        return self._truth[min_bp]


@pytest.fixture(scope="module")
def inbred(gpu_lib):
    fx = Inbred(gpu_lib)
    print("inbred:", fx.figures)
    yield fx
    fx.ctx.close()


def same(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        assert np.array_equal(g, w), f"{what}: {name} differs at {np.argwhere(g != w)[:5].tolist()}"


def test_all_rows_against_all_rows(inbred):
    """device == raster == host build; symmetric; the diagonal is (span, 1, span); a repeat gives the same integers"""
    ctx, want = inbred.ctx, inbred.truth()
    got = ctx.ibd_sharing(0, 0)
    same(got, want, "device against the raster")
    same(inbred.lib.dbg_ibd_host(inbred.parts, inbred.off), want, "host build against the raster")
    for g in got:
        assert np.array_equal(g, g.T)
    assert (np.diag(got[0]) == inbred.span).all() and (np.diag(got[1]) == 1).all() and (np.diag(got[2]) == inbred.span).all()
    same(ctx.ibd_sharing(0, 0), got, "the call repeated")
    r = ibd.sharing(ctx, 0, 0)
    assert r.span_bp == inbred.span
    same(r[1:], want, "ibd.sharing")


def test_min_bp(inbred):
    lengths = sorted({x for row in inbred.segs for s in row for x in s})
    exact = lengths[len(lengths) // 2]                              # some pair's segment length, from the truth
    assert exact > 0
    counted = inbred.truth(exact)[1].astype(np.int64) - inbred.truth(exact + 1)[1].astype(np.int64)
    assert counted.max() >= 1 and counted.min() == 0, "the value is the length of a segment of some pairs and not of others"
    for min_bp in (100_000, exact, exact + 1):
        same(inbred.ctx.ibd_sharing(0, 0, min_bp=min_bp), inbred.truth(min_bp), f"min_bp {min_bp}")
        same(inbred.lib.dbg_ibd_host(inbred.parts, inbred.off, min_bp=min_bp), inbred.truth(min_bp), f"host build, min_bp {min_bp}")


@pytest.mark.parametrize("chunk", [0, 5])
def test_row_ranges_around_the_tile_and_the_wave_block(inbred, chunk):
    """every A range against every B range; chunk 5: sub-blocks of 5 rows a side, whose edges fall inside tiles"""
    ctx, want = inbred.ctx, inbred.truth()
    ctx.dbg_output_chunk(chunk)
    try:
        for a0, na in RANGES:
            for b0, nb in RANGES:
                got = ctx.ibd_sharing(0, 0, a0, na, 0, b0, nb)
                same(got, [w[a0:a0 + na, b0:b0 + nb] for w in want], f"rows [{a0},+{na}) x [{b0},+{nb}), chunk {chunk}")
    finally:
        ctx.dbg_output_chunk(0)


def test_null_outputs(inbred):
    ctx, want = inbred.ctx, inbred.truth()
    for skip in range(3):
        flags = tuple(k != skip for k in range(3))
        outs = ctx.ibd_sharing(0, 0, want=flags)
        assert outs[skip] is None
        same([o for o in outs if o is not None], [w for w, f in zip(want, flags) if f], f"output {NAMES[skip]} null")
    assert ctx.ibd_sharing(0, 0, want=(False, False, False)) == (None, None, None)
    sh = np.full((3, 4), 7, dtype=np.uint64); ns = np.full((3, 4), 7, dtype=np.uint32); mx = np.full((3, 4), 7, dtype=np.uint64)
    for na, nb in ((0, 4), (3, 0), (0, 0)):
        ctx._call("ibd_sharing", 0, 0, 5, na, 0, 9, nb, 0, sh, ns, mx)
        assert (sh == 7).all() and (ns == 7).all() and (mx == 7).all()
    bp, n_parts = ctx.ancestry_bp(0, 0)
    assert np.array_equal(n_parts, np.diff(inbred.off.astype(np.int64))) and (bp[:, 0] == inbred.span).all()
    ctx._call("ancestry_bp", 0, 0, 3, 0, sh, ns)
    assert (sh == 7).all() and (ns == 7).all()
    only_n = np.zeros(5, dtype=np.uint32)
    ctx._call("ancestry_bp", 0, 0, 3, 5, None, only_n)
    assert np.array_equal(only_n, n_parts[3:8])


def test_coancestry_and_inbreeding(inbred):
    """against the raster's fractions, to 1e-15 relative: one float64 division of exact integers"""
    ctx, sh = inbred.ctx, inbred.truth()[0]
    want = T.coancestry_fractions(sh, inbred.span)
    got = ibd.coancestry(ctx, 0)
    assert got.shape == (N, N) and got.dtype == np.float64
    for i in range(N):
        for k in range(N):
            assert abs(Fraction(float(got[i, k])) - want[i][k]) <= want[i][k] * Fraction(1, 10 ** 15), (i, k)
    f = ibd.inbreeding(ctx, 0)
    assert f.shape == (N,)
    for i in range(N):
        w = Fraction(int(sh[2 * i, 2 * i + 1]), inbred.span)
        assert abs(Fraction(float(f[i])) - w) <= w * Fraction(1, 10 ** 15), i
    assert (f > 0).any(), "twelve generations of 40 were meant to leave inbred individuals"
    sub = ibd.coancestry(ctx, 0, ind=(7, 9), min_bp=100_000)
    w100 = T.coancestry_fractions(inbred.truth(100_000)[0][14:32, 14:32], inbred.span)
    assert all(abs(Fraction(float(sub[i, k])) - w100[i][k]) <= w100[i][k] * Fraction(1, 10 ** 15) for i in range(9) for k in range(9))
    assert np.array_equal(ibd.inbreeding(ctx, 0, ind=(7, 9)), f[7:16])
    adm = ibd.admixture(ctx, 0)
    assert adm.shape == (N, 1) and (adm == 1.0).all()


def test_plane_less_context(gpu_lib):
    """the same run without genotype planes: equal to the raster of its own lists; pair_genotype_counts still has nothing to read"""
    ctx, _ = build_inbred(gpu_lib, dense=False)
    parts, off = ctx.download_intervals(0, 0)
    fixture_conditions(parts, off, T.all_segments(parts, off))
    want = T.truth(parts, off)
    same(ctx.ibd_sharing(0, 0), want, "plane-less context")
    same(ctx.ibd_sharing(0, 0, 3, 17, 0, 15, 33, min_bp=100_000), [w[3:20, 15:48] for w in T.truth(parts, off, min_bp=100_000)], "plane-less context, a block")
    with pytest.raises(capi.GevError) as e:
        ctx.pair_genotype_counts(0, 0, 0, 1)
    assert e.value.code == -2 and "no resident genotype planes" in str(e.value)
    ctx.close()


def test_two_populations_behind_a_migration(gpu_lib):
    """populations of 12 and 9 on two chromosomes: two generations, three individuals move from population 0 to 1 and the first call
    comes directly behind the move (it materialises the pending order), three more generations of population 1"""
    from tests.test_gpu_migrant_record import SIZES, scenario
    g, sim, _, _ = scenario(gpu_lib, True, True)
    sim.ras_do_migration([(0, 7, 1), (0, 4, 1), (0, 0, 1)])
    first = [g.ibd_sharing(k, 0, pop_b=1) for k in range(2)]
    assert g.pop_size(0) == SIZES[0] - 3 and g.pop_size(1) == SIZES[1] + 3
    for k in range(2):
        pa, oa = g.download_intervals(0, k); pb, ob = g.download_intervals(1, k)
        same(first[k], T.truth(pa, oa, pb, ob), f"directly behind the migration, chromosome {k}")
    for _ in range(3):
        sim.next_generation_rm(1, SIZES[1] + 3)
    span = [g._span_bp[(1, k)] for k in range(2)]
    both = 0
    for k in range(2):
        pa, oa = g.download_intervals(0, k); pb, ob = g.download_intervals(1, k)
        want = T.truth(pa, oa, pb, ob)
        same(g.ibd_sharing(k, 0, pop_b=1), want, f"population 0 x population 1, chromosome {k}")
        same(g.ibd_sharing(k, 1, 3, 17, 0, 1, 16, min_bp=2000), [w[3:20, 1:17] for w in T.truth(pb, ob, pa, oa, min_bp=2000)], f"population 1 x population 0, a block, chromosome {k}")
        same(gpu_lib.dbg_ibd_host(pa, oa, pb, ob), want, f"host build, chromosome {k}")
        bp, n_parts = g.ancestry_bp(1, k)
        assert bp.shape == (2 * g.pop_size(1), 2) and np.array_equal(n_parts, np.diff(ob.astype(np.int64)))
        for r in range(len(ob) - 1):
            mine = pb[int(ob[r]):int(ob[r + 1])]
            for p in range(2):
                assert int(bp[r, p]) == sum(int(x["en"]) - int(x["st"]) for x in mine if x["root_population"] == p), (k, r, p)
            assert int(bp[r].sum()) == sum(int(x["en"]) - int(x["st"]) for x in mine) == span[k], "a row's columns sum to its covered length"
        both += int(((bp[:, 0] > 0) & (bp[:, 1] > 0)).sum())
    assert both > 0, "population 1 was meant to hold rows that descend from both root populations"
    adm = ibd.admixture(g, 1)
    assert adm.shape == (g.pop_size(1), 2) and np.allclose(adm.sum(axis=1), 1.0, rtol=0, atol=4e-16)
    assert ((adm[:, 0] > 0) & (adm[:, 1] > 0)).any()
    assert (ibd.admixture(g, 0) == [1.0, 0.0]).all()
    g.close()


def test_refusals(gpu_lib):
    """each gives the documented code and leaves the outputs untouched"""
    sh = np.full((2, 2), 7, dtype=np.uint64); ns = np.full((2, 2), 7, dtype=np.uint32); mx = np.full((2, 2), 7, dtype=np.uint64)
    bp = np.full((2, 2), 7, dtype=np.uint64); n_parts = np.full(2, 7, dtype=np.uint32)

    def refused(ctx, code, word, a=(0, 2), b=(0, 2), chr=0):
        for name, args in (("ibd_sharing", (chr, 0, a[0], a[1], 0, b[0], b[1], 0, sh, ns, mx)), ("ancestry_bp", (0, chr, a[0], a[1], bp, n_parts))):
            rc = ctx.L._f(name)(ctx.h, *args)
            assert rc == code and word in ctx.L.last_error(), f"{name}: {rc} {ctx.L.last_error()}"
        assert all((x == 7).all() for x in (sh, ns, mx, bp, n_parts))

    # interval tracking off
    off, _ = build_inbred(gpu_lib)
    off.set_track_intervals(False)
    refused(off, -2, "interval tracking")
    off.close()
    # an inactive chromosome; a population without a current generation
    cfg = SyntheticConfig(N, 64, nchr=2, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.02, mut_per_row=2e-3, n_cv=8, seed=5)
    two = gpu_lib.create(1, 2, 1)
    for c in range(2):
        two.set_rmap(0, c, cfg.rmap_bp, cfg.rmap_prob, cfg.bp_dist); two.set_mutmap(0, c, cfg.mut_bp, cfg.mut_rate)
    two.set_snps(0, 0, cfg.snp_pos)
    two.set_cvs(0, 0, 0, *cfg.cv[0][0], cfg.vd)
    two.set_chr_active(1, False)
    two.synth_founders(0, 0, 2 * N, 31); two.synth_cv_founders(0, 0, 0, 2 * N, 32)
    refused(two, -2, "no current generation")
    two.init_gen0(0, N, 77)
    refused(two, -2, "not active", chr=1)
    # ranges beyond 2 n
    ctx = two
    refused(ctx, -1, "beyond", a=(2 * N - 1, 2))
    refused(ctx, -1, "beyond", a=(2 * N + 1, 0))
    rc = ctx.L._f("ibd_sharing")(ctx.h, 0, 0, 0, 2, 0, 2 * N - 1, 2, 0, sh, ns, mx)
    assert rc == -1 and "rows (b)" in ctx.L.last_error() and (sh == 7).all()
    # between generation_begin and generation_end
    ctx.generation_begin(0, 12345, N)
    try:
        refused(ctx, -2, "pending")
    finally:
        ctx.generation_end()
    assert ctx.ibd_sharing(0, 0)[1].shape == (2 * N, 2 * N)
    two.close()
