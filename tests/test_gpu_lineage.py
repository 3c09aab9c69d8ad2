"""gev_founder_at / gev_founder_counts: the founder of every haplotype row at given positions and the rows by founder per position, walked
on the device from the ancestry interval lists, against the linear scan of tests/lineage_inputs.py on the lists gev_download_intervals
returns and against the same header built for the host: (a) a bred population of 320 rows (the 256-row workgroup and the 64-lane wave
are both crossed), row ranges, position batches of 7, a repeat, a context without genotype planes, turns with ibd_sharing; (b) the
identity that ties sum_sq to the records of ibd.segments; (c) hand-built immigrants of three root populations, once with a founder
count that lays a population across the edge of the count kernel's tile; (d) the refusals (pytest -m gpu)."""
import numpy as np
import pytest

from geneevolve_amd import capi, ibd, lineage
from geneevolve_amd.capi import LINEAGE_SITE_DTYPE, NO_FOUNDER
from geneevolve_amd.host import Simulation, SyntheticConfig
from tests import lineage_inputs as LI
from tests import migrant_inputs as M

pytestmark = pytest.mark.gpu

N, GENS, SEED = 160, 12, 4242
ROWS = 2 * N
RANGES = [(0, 320), (1, 1), (63, 130), (250, 70), (255, 2), (256, 64), (319, 1)]
COUNT_OUTS = ("counts", "site", "pop_counts")


def bred_config():
    return SyntheticConfig(N, 64, nchr=1, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.02, mut_per_row=2e-3, n_cv=8, seed=5)


def build_bred(lib, dense=True):
    """160 individuals bred at random for GENS generations from 320 founder haplotypes, on a context of `lib`"""
    cfg = bred_config()
    ctx = lib.create(1, 1, 1)
    if not dense:
        ctx.set_dense_state(False)
    cfg.apply_static(ctx)
    if dense:
        ctx.synth_founders(0, 0, ROWS, 31)
    ctx.synth_cv_founders(0, 0, 0, ROWS, 32)
    sim = Simulation(ctx, SEED, 1, True)
    sim.ras_initial_human_gen0(0, N)
    for _ in range(GENS):
        sim.next_generation_rm(0, N)
    return ctx


def positions_of(parts):
    """every part boundary and its two neighbours, a regular grid, one position below the map and the last map position"""
    cfg = bred_config()
    lo, hi = int(cfg.rmap_bp[0]), int(cfg.rmap_bp[-1])
    b = np.unique(np.r_[parts["st"], parts["en"]]).astype(np.int64)
    pos = np.unique(np.r_[b - 1, b, b + 1, np.arange(lo, hi, 12_345), lo - 1, hi])
    assert pos.min() >= 0
    return pos.astype(np.uint64)


def fixture_conditions(parts, off, truth):
    """what the cases below need of the population, asserted from the truth -> the figures"""
    per_row = np.diff(off.astype(np.int64))
    site, tie = truth["site"], LI.ties(truth["counts"])
    covered = site["n_covered"] > 0
    fig = {"rows": len(off) - 1, "parts_min": int(per_row.min()), "parts_max": int(per_row.max()), "positions": len(site), "uncovered": int((~covered).sum()),
           "n_lineages_min": int(site["n_lineages"][covered].min()), "n_lineages_max": int(site["n_lineages"].max()), "top_count_max": int(site["top_count"].max()),
           "tied": float((tie[covered] >= 2).mean()), "unique": float((tie[covered] == 1).mean())}
    assert fig["rows"] == ROWS and fig["parts_min"] >= 10, fig
    assert fig["n_lineages_min"] < ROWS // 2, fig
    assert fig["tied"] > 0 and fig["unique"] > 0, fig
    assert fig["uncovered"] >= 2 and (site["n_covered"][covered] == ROWS).all(), fig
    return fig


class Bred:
    def __init__(self, lib):
        self.lib = lib
        self.ctx = build_bred(lib)
        self.parts, self.off = self.ctx.download_intervals(0, 0)
        self.pos = positions_of(self.parts)
        self.nfh = [ROWS]
        self.truth = LI.truth_scan(self.parts, self.off, self.pos, self.nfh)
        for m in self.truth.values():
            m.setflags(write=False)
        self.figures = fixture_conditions(self.parts, self.off, self.truth)
        self.host = dict(zip(LI.OUTPUTS, lib.dbg_lineage_host(self.parts, self.off, self.pos, self.nfh)))

    def rows(self, r0, n, every=1):
        """the truth over rows [r0, +n) at every `every`-th position: the columns of fid, the rest counted from them"""
        if (r0, n, every) == (0, ROWS, 1):
            return self.truth
        return LI.from_fid(np.ascontiguousarray(self.truth["fid"][::every, r0:r0 + n]), self.nfh)


@pytest.fixture(scope="module")
def bred(gpu_lib):
    fx = Bred(gpu_lib)
    print("bred:", fx.figures)
    yield fx
    fx.ctx.close()


def device(ctx, pos, r0=0, n=None, nfh=None):
    return {"fid": ctx.founder_at(0, 0, pos, r0, n, nfh), **dict(zip(COUNT_OUTS, ctx.founder_counts(0, 0, pos, r0, n, nfh)))}


# ---- (a) the bred population ---------------------------------------------------------------------------------------------------------------
def test_all_rows(bred):
    """device == linear scan == host build, all four outputs; a repeat gives the same bytes; the wrapper's founder count is the default"""
    assert bred.ctx.founder_haps().tolist() == bred.nfh
    got = device(bred.ctx, bred.pos)
    LI.same(got, bred.truth, "device against the linear scan")
    LI.same(bred.host, bred.truth, "host build against the linear scan")
    again = device(bred.ctx, bred.pos)
    assert all(again[k].tobytes() == got[k].tobytes() for k in LI.OUTPUTS), "the call repeated"
    site = got["site"]
    assert np.array_equal(got["counts"].sum(axis=1), site["n_covered"]) and np.array_equal(got["pop_counts"][:, 0], site["n_covered"])


@pytest.mark.parametrize("chunk", [0, 7])
def test_row_ranges_around_the_workgroup_and_the_wave(bred, chunk):
    """chunk 7: batches of 7 positions (every third position: the batches' edges fall between duplicates of nothing and anywhere)"""
    ctx, every = bred.ctx, 3 if chunk else 1
    pos = np.ascontiguousarray(bred.pos[::every])
    ctx.dbg_output_chunk(chunk)
    try:
        for r0, n in RANGES:
            want = bred.rows(r0, n, every)
            LI.same(device(ctx, pos, r0, n), want, f"rows [{r0},+{n}), chunk {chunk}")
            p, o = bred.parts[int(bred.off[r0]):int(bred.off[r0 + n])], (bred.off[r0:r0 + n + 1] - bred.off[r0]).astype(np.uint64)
            LI.same(bred.lib.dbg_lineage_host(p, o, pos, bred.nfh), want, f"host build, rows [{r0},+{n})")
    finally:
        ctx.dbg_output_chunk(0)


def test_null_outputs_and_empty_requests(bred):
    ctx, pos = bred.ctx, np.ascontiguousarray(bred.pos[::5])
    want = bred.rows(0, ROWS, 5)
    for skip in COUNT_OUTS:
        names = tuple(k for k in COUNT_OUTS if k != skip)
        outs = dict(zip(COUNT_OUTS, ctx.founder_counts(0, 0, pos, want=names)))
        assert outs[skip] is None
        LI.same(outs, want, f"output {skip} null")
    assert ctx.founder_counts(0, 0, pos, want=()) == (None, None, None)
    fid = np.full((2, 3), 7, dtype=np.uint32); counts = np.full((2, ROWS), 7, dtype=np.uint32); site = np.zeros(2, dtype=LINEAGE_SITE_DTYPE); pc = np.full((2, 1), 7, dtype=np.uint32)
    site["n_lineages"] = 7
    nfh = np.array(bred.nfh, dtype=np.uint64)
    ctx._call("founder_at", 0, 0, 5, 3, pos, 0, nfh, fid)
    ctx._call("founder_at", 0, 0, 5, 0, pos, 2, nfh, fid)
    ctx._call("founder_counts", 0, 0, 5, 3, pos, 0, nfh, counts, site, pc)
    assert (fid == 7).all() and (counts == 7).all() and (site["n_lineages"] == 7).all() and (pc == 7).all()
    ctx._call("founder_counts", 0, 0, 5, 0, pos, 2, nfh, counts, site, pc)
    assert not counts.any() and not pc.any() and [s.tolist() for s in site] == [(0, 0, 0, 0, NO_FOUNDER)] * 2


def test_module_over_unsorted_positions(bred):
    """lineage.py sorts the positions and returns the caller's order; its reductions are one division of the device's integers"""
    rs = np.random.RandomState(2)
    pick = rs.permutation(len(bred.pos))[:200]
    pos = bred.pos[pick]
    assert (np.diff(pos.astype(np.int64)) < 0).any()
    assert np.array_equal(lineage.at(bred.ctx, 0, 0, pos), bred.truth["fid"][pick])
    assert np.array_equal(lineage.at(bred.ctx, 0, 0, pos, rows=(63, 130)), bred.truth["fid"][pick, 63:193])
    site, pc = lineage.sites(bred.ctx, 0, 0, pos)
    assert site.tobytes() == bred.truth["site"][pick].tobytes() and np.array_equal(pc, bred.truth["pop_counts"][pick])
    la = lineage.local_ancestry(bred.ctx, 0, 0, pos, ind=(7, 9))
    cov = bred.truth["fid"][pick][:, 14:32] != NO_FOUNDER
    assert la.dtype == np.uint8 and la.shape == (9, 200, 1) and np.array_equal(la[:, :, 0], (cov[:, 0::2].astype(np.uint8) + cov[:, 1::2]).T)
    n, s = site["n_covered"].astype(np.float64), site["sum_sq"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(lineage.founder_genome_equivalents(site), np.where(n > 0, n * n / s, np.nan), equal_nan=True)
        assert np.array_equal(lineage.ibd_probability(site), np.where(n > 1, (s - n) / (n * (n - 1)), np.nan), equal_nan=True)
    freq = lineage.ancestry_frequency(site, pc)
    assert np.array_equal(np.isnan(freq[:, 0]), n == 0) and (freq[n > 0] == 1.0).all()


def test_plane_less_context_and_turns_with_ibd_sharing(gpu_lib):
    """the same run without genotype planes: equal to the scan of its own lists; an ibd_sharing call between two lineage calls changes
    neither"""
    ctx = build_bred(gpu_lib, dense=False)
    assert ctx.founder_haps().tolist() == [ROWS]                        # (from the CV founders: there are no genotype founders here)
    parts, off = ctx.download_intervals(0, 0)
    pos = np.ascontiguousarray(positions_of(parts)[::4])
    want = LI.truth_scan(parts, off, pos, [ROWS])
    first = device(ctx, pos)
    LI.same(first, want, "plane-less context")
    sh = ctx.ibd_sharing(0, 0, 3, 17, 0, 15, 33)
    again = device(ctx, pos)
    assert all(again[k].tobytes() == first[k].tobytes() for k in LI.OUTPUTS)
    assert all(np.array_equal(a, b) for a, b in zip(ctx.ibd_sharing(0, 0, 3, 17, 0, 15, 33), sh))
    with pytest.raises(capi.GevError) as e:
        ctx.pair_genotype_counts(0, 0, 0, 1)
    assert e.value.code == -2 and "no resident genotype planes" in str(e.value)
    ctx.close()


# ---- (b) the identity between the two readings of the lists ----------------------------------------------------------------------------------
def test_sum_sq_counts_the_ibd_segments_over_a_position(bred):
    """at 50 positions: the pairs of rows with one founder, (sum_sq - n_covered) / 2, are the records of ibd.segments (pairs a < b)
    with st <= x < en"""
    pos = np.ascontiguousarray(bred.pos[np.linspace(0, len(bred.pos) - 1, 50).astype(int)])
    site, _ = lineage.sites(bred.ctx, 0, 0, pos)
    seg = ibd.segments(bred.ctx, 0)
    assert len(seg) > ROWS and (seg["row_a"] < seg["row_b"]).all()
    pairs = [int(((seg["st"] <= x) & (x < seg["en"])).sum()) for x in pos]
    assert (site["sum_sq"].astype(np.int64) - site["n_covered"]).tolist() == [2 * k for k in pairs]
    assert max(pairs) > 0 and pairs[0] == 0 and pairs[-1] == 0         # (below the map and at its last position nothing is covered)


# ---- (c) hand-built immigrants, and a population across the tile edge ---------------------------------------------------------------------------
def test_immigrants_of_three_root_populations(gpu_lib):
    """imported as test_gpu_migrant_import.py imports them; every boundary of the immigrants' lists and its neighbours; all rows of the
    population (residents and immigrants) and the immigrants alone.  Declaring population 0 with gev_dbg_lineage_tile() - 14 founders
    lays the 24 founders of population 1 across the first tile's edge: two tiles, their partials folded by the finish kernel, with
    counts on both sides"""
    from tests.test_gpu_migrant_import import N0, N_IMM, device_context, import_record, start
    g, _ = device_context(gpu_lib, "copied")
    start(g, False)
    import_record(g, M.encode(M.IMMIGRANTS, True), N_IMM)
    real = [M.n_founders(p) for p in range(M.N_POP)]
    assert g.founder_haps().tolist() == real == [28, 24, 32]
    pos = np.array(LI.boundary_positions([parts for parts, _ in M.rows_of(M.IMMIGRANTS, 0)]), dtype=np.uint64)
    assert len(pos) == 1560
    parts, off = g.download_intervals(0, 0)
    r_imm, n_all = 2 * N0, 2 * (N0 + N_IMM)
    tile = gpu_lib.dbg_lineage_tile()
    assert gpu_lib.dbg_lineage_tile() == tile and tile - 14 >= real[0]
    for nfh, every in ((real, 1), ([tile - 14, real[1], real[2]], 8)):
        p = np.ascontiguousarray(pos[::every])
        want = LI.truth_scan(parts, off, p, nfh)
        if every == 1:
            LI.same(LI.truth([q for q, _ in M.rows_of(M.IMMIGRANTS, 0)], p.tolist(), nfh), LI.from_fid(np.ascontiguousarray(want["fid"][:, r_imm:]), nfh), "the scans agree")
        else:
            used = np.flatnonzero(want["counts"].any(axis=0))
            assert (used < tile).any() and (used >= tile).any() and ((used >= tile - 14) & (used < tile)).any(), "counts on both sides of the tile edge"
            both = (want["counts"][:, :tile] != 0).any(axis=1) & (want["counts"][:, tile:] != 0).any(axis=1)
            assert both.any() and (want["site"]["n_lineages"][both] >= 2).all()
        got = {"fid": g.founder_at(0, 0, p, n_founder_haps=nfh), **dict(zip(COUNT_OUTS, g.founder_counts(0, 0, p, n_founder_haps=nfh)))}
        LI.same(got, want, f"all rows, founder counts {nfh}")
        LI.same(gpu_lib.dbg_lineage_host(parts, off, p, nfh), want, f"host build, founder counts {nfh}")
        imm = LI.from_fid(np.ascontiguousarray(want["fid"][:, r_imm:]), nfh)
        got = {"fid": g.founder_at(0, 0, p, r_imm, n_all - r_imm, nfh), **dict(zip(COUNT_OUTS, g.founder_counts(0, 0, p, r_imm, n_all - r_imm, nfh)))}
        LI.same(got, imm, f"the immigrants' rows, founder counts {nfh}")
        g.dbg_output_chunk(7)
        try:
            site, pc = g.founder_counts(0, 0, p[:40], n_founder_haps=nfh, want=("site", "pop_counts"))[1:]
        finally:
            g.dbg_output_chunk(0)
        assert site.tobytes() == want["site"][:40].tobytes() and np.array_equal(pc, want["pop_counts"][:40]), f"batches of 7, founder counts {nfh}"
    dosage = lineage.local_ancestry(g, 0, 0, pos[::8], ind=(N0, N_IMM))
    rp, _ = lineage.labels(LI.truth_scan(parts, off, pos[::8], real, want_counts=False)["fid"][:, r_imm:], real)
    assert dosage.shape == (N_IMM, len(pos[::8]), 3) and dosage.max() == 2
    for q in range(3):
        assert np.array_equal(dosage[:, :, q], ((rp[:, 0::2] == q).astype(np.uint8) + (rp[:, 1::2] == q)).T)
    g.close()


# ---- (d) the refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(bred, gpu_lib):
    """the device calls refuse what the host form refuses, in the same words, and write nothing; GEV_ESTATE as gev_ibd_sharing gives it"""
    fid = np.full((3, 2), 7, dtype=np.uint32); counts = np.full((3, ROWS), 7, dtype=np.uint32); site = np.zeros(3, dtype=LINEAGE_SITE_DTYPE); pc = np.full((3, 1), 7, dtype=np.uint32)
    site["top_count"] = 7
    parts, off = bred.parts[:int(bred.off[2])], bred.off[:3]
    big_hap = int(max(bred.parts["hap_index"][:int(bred.off[2])]))

    def untouched():
        assert (fid == 7).all() and (counts == 7).all() and (site["top_count"] == 7).all() and (pc == 7).all()

    def both(ctx, pos, nfh, a=(0, 2)):
        """(code, message with the call's name taken out) of the two device calls, which must agree"""
        pos = None if pos is None else np.array(pos, dtype=np.uint64); nfh = None if nfh is None else np.array(nfh, dtype=np.uint64)
        n_pos = 3 if pos is None else len(pos)
        out = []
        for name, tail in (("founder_at", (fid,)), ("founder_counts", (counts, site, pc))):
            rc = ctx.L._f(name)(ctx.h, 0, 0, a[0], a[1], pos, n_pos, nfh, *tail)
            msg = ctx.L.last_error()
            out.append((rc, msg[len(name) + 2:] if msg.startswith(name + ": ") else msg))      # (a pending generation's message names no call)
        untouched()
        assert out[0] == out[1]
        return out[0]

    def host(pos, nfh):
        pos = None if pos is None else np.array(pos, dtype=np.uint64); nfh = None if nfh is None else np.array(nfh, dtype=np.uint64)
        rc = gpu_lib._f("dbg_lineage_host")(parts, off, 2, pos, 3 if pos is None else len(pos), nfh, 1, fid, counts, site, pc)
        msg = gpu_lib.last_error()
        untouched()
        assert msg.startswith("dbg_lineage_host: ")
        return rc, msg[len("dbg_lineage_host: "):]

    ctx = bred.ctx
    for pos, nfh, code in (([5000, 7000, 6999], [ROWS], -1), ([5000, 6000, 7000], [big_hap], -1), ([5000, 6000, 7000], [(1 << 32) - 1], -5), ([5000, 6000, 7000], None, -1),
                           (None, [ROWS], -1)):
        got = both(ctx, pos, nfh)
        assert got[0] == code and got == host(pos, nfh), (pos, nfh, got)
    assert "decrease at index 2 (6999 behind 7000)" in both(ctx, [5000, 7000, 6999], [ROWS])[1]
    assert both(ctx, [5000, 6000, 7000], [ROWS], a=(ROWS - 1, 2)) == (-1, f"rows [{ROWS - 1},{ROWS + 1}) beyond the {ROWS} there are")
    rc = ctx.L._f("founder_at")(ctx.h, 0, 0, 0, 2, np.array([5, 6, 7], dtype=np.uint64), 3, np.array([ROWS], dtype=np.uint64), None)
    assert (rc, ctx.L.last_error()) == (-1, "founder_at: fid is null")

    def as_ibd_sharing(c):
        sh = np.full((2, 2), 7, dtype=np.uint64)
        rc = c.L._f("ibd_sharing")(c.h, 0, 0, 0, 2, 0, 0, 2, 0, sh, None, None)
        msg = c.L.last_error()
        assert rc == -2 and (sh == 7).all()
        return rc, msg[len("ibd_sharing: "):] if msg.startswith("ibd_sharing: ") else msg

    # a population without a current generation
    off_ctx = gpu_lib.create(1, 1, 1)
    cfg = SyntheticConfig(20, 64, nchr=1, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.02, mut_per_row=2e-3, n_cv=8, seed=5)
    cfg.apply_static(off_ctx)
    off_ctx.synth_founders(0, 0, 40, 31); off_ctx.synth_cv_founders(0, 0, 0, 40, 32)
    got = both(off_ctx, [5000, 6000, 7000], [40])
    assert got[0] == -2 and "no current generation" in got[1] and got == as_ibd_sharing(off_ctx)
    off_ctx.init_gen0(0, 20, 77)
    p0, o0 = off_ctx.download_intervals(0, 0)
    assert np.array_equal(off_ctx.founder_at(0, 0, [5000, 6000]), LI.truth_scan(p0, o0, [5000, 6000], [40])["fid"])
    # between generation_begin and generation_end
    off_ctx.generation_begin(0, 12345, 20)
    try:
        got = both(off_ctx, [5000, 6000, 7000], [40])
        want = as_ibd_sharing(off_ctx)
    finally:
        off_ctx.generation_end()
    assert got[0] == -2 and "pending" in got[1] and got == want
    assert off_ctx.founder_counts(0, 0, [5000], want=("site",))[1]["n_covered"].tolist() == [40]
    # interval tracking off
    off_ctx.set_track_intervals(False)
    got = both(off_ctx, [5000, 6000, 7000], [40])
    assert got == (-2, "interval tracking is disabled (gev_set_track_intervals)") and got == as_ibd_sharing(off_ctx)
    off_ctx.close()
