"""gev_ibd_segments: the IBD segments of pairs of haplotype rows listed on the device in (row_a, row_b, st) order, against the runs of the
raster (tests/ibd_segments_inputs.py) on the lists gev_download_intervals returns and against the same header built for the host: the
inbred population of test_gpu_ibd.py in both pair modes, row ranges around the tile and the wave block under strips of any, 5 and 1
rows, thresholds, a repeat, consistency with gev_ibd_sharing, the capacity rule with a guard, empty ranges, a context without genotype
planes, two populations behind a migration, and the refusals (pytest -m gpu).  Every comparison is equality of the bytes."""
import ctypes as C

import numpy as np
import pytest

from geneevolve_amd import capi, ibd
from geneevolve_amd.capi import IBD_ALL_PAIRS, IBD_UPPER, SEGMENT_DTYPE
from geneevolve_amd.host import SyntheticConfig
from tests import ibd_segments_inputs as S
from tests.test_gpu_ibd import N, RANGES, build_inbred, fixture_conditions

pytestmark = pytest.mark.gpu


def segment_conditions(runs):
    """what the cases below need of a population, asserted from the truth -> the figures"""
    nseg = np.array([[len(r) for r in row] for row in runs])
    flat = nseg.ravel()
    with_seg = np.flatnonzero(flat > 0)
    inside = flat[with_seg[0]:with_seg[-1] + 1]
    n_all, n_upper = int(nseg.sum()), int(np.triu(nseg, 1).sum())
    fig = {"records": n_all, "upper": n_upper, "empty_between": int((inside == 0).sum()), "most": int(nseg.max())}
    assert fig["empty_between"] >= 1, fig
    assert fig["most"] >= 5, fig
    assert 0 < 2 * n_upper < n_all, fig
    return fig


class Inbred:
    def __init__(self, lib, dense=True):
        self.lib = lib
        self.ctx, self.sim = build_inbred(lib, dense=dense)
        self.parts, self.off = self.ctx.download_intervals(0, 0)
        self.n = len(self.off) - 1
        self.runs = S.all_runs(self.parts, self.off)
        fixture_conditions(self.parts, self.off, [[[en - st for st, en in r] for r in row] for row in self.runs])
        self.figures = segment_conditions(self.runs)
        self.lengths = sorted({en - st for row in self.runs for r in row for st, en in r})

    def truth(self, a=None, b=None, min_bp=0, upper=False):
        """the raster's records of rows a x rows b, named by their absolute rows"""
        return S.records(self.runs, min_bp, upper, a, b)

    def host(self, a=None, b=None, min_bp=0, upper=False):
        """the host build on the downloaded lists of the two ranges; its row indices are moved to the absolute rows"""
        a = (0, self.n) if a is None else a; b = (0, self.n) if b is None else b
        rec = self.lib.dbg_ibd_segments_host(self.parts, self.off[a[0]:a[0] + a[1] + 1], self.parts, self.off[b[0]:b[0] + b[1] + 1], min_bp)
        rec["row_a"] += a[0]; rec["row_b"] += b[0]
        return rec[rec["row_a"] < rec["row_b"]] if upper else rec

    def check(self, what, a=None, b=None, min_bp=0, upper=False):
        a_ = (0, self.n) if a is None else a; b_ = (0, self.n) if b is None else b
        want = self.truth(a, b, min_bp, upper)
        got = self.ctx.ibd_segments(0, 0, a_[0], a_[1], 0, b_[0], b_[1], min_bp, upper)
        S.same(got, want, f"device against the raster, {what}")
        S.same(self.host(a, b, min_bp, upper), want, f"host build against the raster, {what}")
        return got


@pytest.fixture(scope="module")
def inbred(gpu_lib):
    fx = Inbred(gpu_lib)
    print("inbred:", fx.figures)
    yield fx
    fx.ctx.close()


def min_bps(lengths):
    """0, an occurring length, that plus one, one beyond every segment"""
    exact = lengths[len(lengths) // 2]
    return (0, exact, exact + 1, lengths[-1] + 1)


def test_all_rows_against_all_rows(inbred):
    for upper in (False, True):
        got = inbred.check(f"all rows, upper {upper}", upper=upper)
        assert len(got) == inbred.figures["upper" if upper else "records"]
        again = inbred.ctx.ibd_segments(0, 0, upper=upper)
        assert again.tobytes() == got.tobytes(), "the call repeated"
    # the same population's host form in UPPER mode on the whole list, where its row indices are the rows
    S.same(inbred.lib.dbg_ibd_segments_host(inbred.parts, inbred.off, upper=True), inbred.truth(upper=True), "host build, upper")
    seg = ibd.segments(inbred.ctx, 0)
    assert seg.dtype.names == ("chr", "st", "en", "row_a", "row_b") and (seg["chr"] == 0).all()
    want = inbred.truth(upper=True)
    assert all(np.array_equal(seg[name], want[name]) for name in SEGMENT_DTYPE.names), "ibd.segments defaults to the upper triangle"
    ia, ca, ib, cb = ibd.segment_individuals(seg)
    assert np.array_equal(2 * ia + ca, seg["row_a"]) and np.array_equal(2 * ib + cb, seg["row_b"]) and ia.max() < N
    rect = ibd.segments(inbred.ctx, 0, rows=(3, 17), rows_b=(15, 33))
    assert all(np.array_equal(rect[name], inbred.truth((3, 17), (15, 33))[name]) for name in SEGMENT_DTYPE.names), "other rows: all pairs"


@pytest.mark.parametrize("chunk", [0, 5, 1])
def test_row_ranges_around_the_tile_and_the_wave_block(inbred, chunk):
    """every A range against every B range; chunk 5: strips of 5 A rows, whose edges fall inside tiles; chunk 1: single rows"""
    inbred.ctx.dbg_output_chunk(chunk)
    try:
        for a in RANGES:
            for b in RANGES:
                inbred.check(f"rows [{a[0]},+{a[1]}) x [{b[0]},+{b[1]}), chunk {chunk}", a, b)
    finally:
        inbred.ctx.dbg_output_chunk(0)


@pytest.mark.parametrize("chunk", [0, 5, 1])
def test_upper_on_overlapping_ranges(inbred, chunk):
    inbred.ctx.dbg_output_chunk(chunk)
    try:
        for a, b in (((3, 17), (15, 33)), ((15, 33), (3, 17)), ((0, 80), (64, 16)), ((64, 16), (0, 80)), ((79, 1), (0, 80)), ((3, 17), (3, 17))):
            got = inbred.check(f"upper, rows [{a[0]},+{a[1]}) x [{b[0]},+{b[1]}), chunk {chunk}", a, b, upper=True)
            assert (got["row_a"] < got["row_b"]).all()
        assert len(inbred.ctx.ibd_segments(0, 0, 40, 20, 0, 10, 30, upper=True)) == 0, "a block wholly below the diagonal"
    finally:
        inbred.ctx.dbg_output_chunk(0)


def test_min_bp(inbred):
    values = min_bps(inbred.lengths)
    at, above = inbred.truth(min_bp=values[1]), inbred.truth(min_bp=values[2])
    assert len(at) > len(above) > 0, "the value is the length of a segment"
    for upper in (False, True):
        for min_bp in values:
            got = inbred.check(f"min_bp {min_bp}, upper {upper}", min_bp=min_bp, upper=upper)
            assert (len(got) == 0) == (min_bp == values[3])


def test_consistency_with_ibd_sharing(inbred):
    """per pair: the records' number, summed length and longest are the three matrices of gev_ibd_sharing"""
    for min_bp in min_bps(inbred.lengths)[:3]:
        sh, ns, mx = inbred.ctx.ibd_sharing(0, 0, 3, 33, 0, 1, 79, min_bp=min_bp)
        cnt, tot, longest = S.per_pair(inbred.ctx.ibd_segments(0, 0, 3, 33, 0, 1, 79, min_bp), 33, 79, 3, 1)
        assert cnt == ns.tolist() and tot == [[int(x) for x in r] for r in sh] and longest == [[int(x) for x in r] for r in mx]


@pytest.mark.parametrize("chunk", [0, 5])
def test_capacity(inbred, chunk):
    """count-only, exact, one short and two to spare through the raw call: nothing at or beyond out[capacity] is written"""
    ctx = inbred.ctx
    f = ctx.L._f("ibd_segments")
    ctx.dbg_output_chunk(chunk)
    try:
        S.capacity_cases(f, (ctx.h, 0, 0, 0, 80, 0, 0, 80, 0, IBD_ALL_PAIRS), inbred.truth())
        S.capacity_cases(f, (ctx.h, 0, 0, 3, 17, 0, 15, 33, 100_000, IBD_UPPER), inbred.truth((3, 17), (15, 33), 100_000, True))
        rc, n, buf = S.raw(f, (ctx.h, 0, 0, 0, 80, 0, 0, 80, inbred.lengths[-1] + 1, IBD_ALL_PAIRS), 4)
        assert rc == 0 and n == 0 and (buf == S.SENTINEL).all(), "a threshold beyond every segment"
    finally:
        ctx.dbg_output_chunk(0)


def test_empty_ranges(inbred):
    ctx = inbred.ctx
    f = ctx.L._f("ibd_segments")
    for na, nb in ((0, 4), (3, 0), (0, 0)):
        for pairs in (IBD_ALL_PAIRS, IBD_UPPER):
            rc, n, buf = S.raw(f, (ctx.h, 0, 0, 5, na, 0, 9, nb, 0, pairs), 4)
            assert rc == 0 and n == 0 and (buf == S.SENTINEL).all()
    assert len(ctx.ibd_segments(0, 0, 5, 0, 0, 9, 4)) == 0 and len(ctx.ibd_segments(0, 0, 2 * N, 0)) == 0


def test_plane_less_context(gpu_lib):
    fx = Inbred(gpu_lib, dense=False)
    try:
        fx.check("plane-less context")
        fx.check("plane-less context, a block", (3, 17), (15, 33), 100_000, True)
    finally:
        fx.ctx.close()


def test_two_populations_behind_a_migration(gpu_lib):
    """populations of 12 and 9 on two chromosomes: two generations, three individuals move from population 0 to 1 and the first call
    comes directly behind the move (it materialises the pending order), three more generations of population 1"""
    from tests.test_gpu_migrant_record import SIZES, scenario
    g, sim, _, _ = scenario(gpu_lib, True, True)
    try:
        sim.ras_do_migration([(0, 7, 1), (0, 4, 1), (0, 0, 1)])
        first = [g.ibd_segments(k, 0, pop_b=1) for k in range(2)]
        assert g.pop_size(0) == SIZES[0] - 3 and g.pop_size(1) == SIZES[1] + 3
        for k in range(2):
            pa, oa = g.download_intervals(0, k); pb, ob = g.download_intervals(1, k)
            S.same(first[k], S.records(S.all_runs(pa, oa, pb, ob)), f"directly behind the migration, chromosome {k}")
            assert len(first[k]) > 0
        for _ in range(3):
            sim.next_generation_rm(1, SIZES[1] + 3)
        per_chr = []
        for k in range(2):
            pa, oa = g.download_intervals(0, k); pb, ob = g.download_intervals(1, k)
            ab, ba = S.all_runs(pa, oa, pb, ob), S.all_runs(pb, ob, pa, oa)
            want = S.records(ab)
            S.same(g.ibd_segments(k, 0, pop_b=1), want, f"population 0 x population 1, chromosome {k}")
            S.same(gpu_lib.dbg_ibd_segments_host(pa, oa, pb, ob), want, f"host build, chromosome {k}")
            S.same(g.ibd_segments(k, 1, pop_b=0), S.records(ba), f"population 1 x population 0, chromosome {k}")
            S.same(g.ibd_segments(k, 1, 3, 17, 0, 1, 16, min_bp=2000), S.records(ba, 2000, a=(3, 17), b=(1, 16)), f"population 1 x population 0, a block, chromosome {k}")
            per_chr.append(want)
        both = ibd.segments(g, 0, pop_b=1)
        assert both["chr"].tolist() == [0] * len(per_chr[0]) + [1] * len(per_chr[1]) and len(per_chr[0]) and len(per_chr[1])
        for k in range(2):
            mine = both[both["chr"] == k]
            assert all(np.array_equal(mine[name], per_chr[k][name]) for name in SEGMENT_DTYPE.names)
        p1 = ibd.segments(g, 1, chrs=[1, 0])
        pb0, ob0 = g.download_intervals(1, 0); pb1, ob1 = g.download_intervals(1, 1)
        want1 = ibd.segments_over_chromosomes([0, 1], [S.records(S.all_runs(pb0, ob0), upper=True), S.records(S.all_runs(pb1, ob1), upper=True)])
        assert p1.tobytes() == want1.tobytes(), "one population over both chromosomes: the upper triangle, chromosomes ascending"
        # GEV_IBD_UPPER across populations
        out = np.full(4 * SEGMENT_DTYPE.itemsize, S.SENTINEL, dtype=np.uint8); n = C.c_uint64(12345)
        rc = g.L._f("ibd_segments")(g.h, 0, 0, 0, 2, 1, 0, 2, 0, IBD_UPPER, capi._p(out), 4, C.byref(n))
        assert rc == -1 and "one population" in g.L.last_error() and (out == S.SENTINEL).all() and n.value == 12345
    finally:
        g.close()


def test_refusals(gpu_lib):
    """each gives the documented code and leaves out and n_total untouched"""
    out = np.full(8 * SEGMENT_DTYPE.itemsize, S.SENTINEL, dtype=np.uint8)

    def refused(ctx, code, word, a=(0, 2), b=(0, 2), chr=0, pairs=IBD_ALL_PAIRS, n_total=True, capacity=8, null_out=False):
        n = C.c_uint64(12345)
        rc = ctx.L._f("ibd_segments")(ctx.h, chr, 0, a[0], a[1], 0, b[0], b[1], 0, pairs, None if null_out else capi._p(out), capacity, C.byref(n) if n_total else None)
        assert rc == code and word in ctx.L.last_error(), f"{rc} {ctx.L.last_error()}"
        assert (out == S.SENTINEL).all() and n.value == 12345

    # interval tracking off
    off, _ = build_inbred(gpu_lib)
    off.set_track_intervals(False)
    refused(off, -2, "interval tracking")
    off.close()
    # an inactive chromosome; a population without a current generation
    cfg = SyntheticConfig(N, 64, nchr=2, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.02, mut_per_row=2e-3, n_cv=8, seed=5)
    two = gpu_lib.create(1, 2, 1)
    try:
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
        refused(two, -1, "beyond", a=(2 * N - 1, 2))
        refused(two, -1, "beyond", a=(2 * N + 1, 0))
        refused(two, -1, "rows (b)", b=(2 * N - 1, 2))
        # the list's own arguments
        refused(two, -1, "n_total", n_total=False)
        refused(two, -1, "pairs", pairs=2)
        refused(two, -1, "null output", null_out=True, capacity=3)
        # between generation_begin and generation_end
        two.generation_begin(0, 12345, N)
        try:
            refused(two, -2, "pending")
        finally:
            two.generation_end()
        parts, offs = two.download_intervals(0, 0)
        S.same(two.ibd_segments(0, 0, upper=True), gpu_lib.dbg_ibd_segments_host(parts, offs, upper=True), "after generation_end")
    finally:
        two.close()
