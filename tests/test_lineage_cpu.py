"""gev_dbg_lineage_host: the cursor walk and the reductions of geneevolve_amd/csrc/gev_lineage.h compiled for the host, against the linear
scan of tests/lineage_inputs.py on constructed lists, on seeded random rows and on the hand-built immigrants of tests/migrant_inputs.py;
its refusals with their whole messages; the reductions of geneevolve_amd/lineage.py against exact fractions.  No device is needed."""
import math
from fractions import Fraction

import numpy as np
import pytest

from geneevolve_amd import capi, lineage
from geneevolve_amd.capi import LINEAGE_SITE_DTYPE, NO_FOUNDER
from tests import ibd_inputs as T
from tests import lineage_inputs as LI
from tests import migrant_inputs as M

BIG = 1 << 63
TOP = (1 << 64) - 1


def check(gpu_lib, rows, pos, nfh, want=LI.OUTPUTS):
    """the host build on the lists against the linear scan, every output asked for -> the truth"""
    parts, off = T.lists_of([[list(q) for q in row] for row in rows])
    truth = LI.truth(rows, pos, nfh)
    got = gpu_lib.dbg_lineage_host(parts, off, pos, nfh, want=want)
    assert all((g is None) == (name not in want) for g, name in zip(got, LI.OUTPUTS))
    LI.same(got, truth, "host build against the linear scan")
    LI.same(LI.truth_scan(parts, off, pos, nfh), truth, "the scan vectorised over the positions (the GPU tests' truth) against the Python loop")
    return truth


# name: (rows, n_founder_haps, positions, {position index: expected fid of row 0})
CASES = {
    "on st, on en before a gap, on en of a touching part": ([[(10, 20, 1, 0), (25, 30, 2, 0), (30, 40, 3, 0)]], [4], [10, 19, 20, 24, 25, 29, 30, 39],
                                                           {0: 1, 1: 1, 2: NO_FOUNDER, 3: NO_FOUNDER, 4: 2, 5: 2, 6: 3, 7: 3}),
    "before the first part and behind the last": ([[(10, 20, 1, 0), (20, 40, 0, 0)]], [2], [0, 9, 10, 39, 40, 41, TOP], {0: NO_FOUNDER, 1: NO_FOUNDER, 2: 1, 3: 0, 4: NO_FOUNDER, 5: NO_FOUNDER, 6: NO_FOUNDER}),
    "a row without parts": ([[], [(10, 20, 1, 0)], []], [2], [5, 10, 15, 20], {0: NO_FOUNDER, 1: NO_FOUNDER, 2: NO_FOUNDER, 3: NO_FOUNDER}),
    "zero-length and inverted parts": ([[(10, 20, 1, 0), (20, 20, 5, 0), (30, 20, 6, 0), (30, 40, 2, 0), (40, 40, 7, 0)]], [8], [19, 20, 25, 29, 30, 39, 40],
                                       {0: 1, 1: NO_FOUNDER, 2: NO_FOUNDER, 3: NO_FOUNDER, 4: 2, 5: 2, 6: NO_FOUNDER}),
    "duplicate positions": ([[(10, 20, 1, 0), (20, 30, 0, 0)]], [2], [10, 10, 19, 19, 19, 20, 20, 30, 30], {0: 1, 1: 1, 4: 1, 5: 0, 6: 0, 7: NO_FOUNDER, 8: NO_FOUNDER}),
    "positions around 2^63 and at 2^64 - 1": ([[(BIG - 5, BIG, 1, 0), (BIG, TOP, 2, 0)], [(0, BIG + 1, 0, 0)]], [3], [BIG - 6, BIG - 1, BIG, BIG + 1, TOP - 1, TOP],
                                              {0: NO_FOUNDER, 1: 1, 2: 2, 3: 2, 4: 2, 5: NO_FOUNDER}),
    "the same hap_index under two root populations": ([[(10, 20, 3, 0), (20, 30, 3, 1)], [(10, 30, 3, 1)]], [4, 6], [15, 25], {0: 3, 1: 7}),
    "a hap_index of 0 in the last root population": ([[(10, 20, 0, 2)]], [5, 0, 1], [10], {0: 5}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_lists(gpu_lib, name):
    rows, nfh, pos, expect = CASES[name]
    truth = check(gpu_lib, rows, pos, nfh)
    for p, f in expect.items():
        assert int(truth["fid"][p, 0]) == f, (name, p)


def test_a_tie_for_the_top_goes_to_the_lowest_founder(gpu_lib):
    """founders 5 and 2 with two rows each, founder 7 with one; behind position 20 founder 2 loses a row and 5 is alone on top"""
    rows = [[(10, 30, 5, 0)], [(10, 20, 2, 0)], [(10, 30, 7, 0)], [(10, 30, 2, 0)], [(10, 30, 5, 0)]]
    truth = check(gpu_lib, rows, [15, 25, 35], [8])
    assert truth["site"][0].tolist() == (9, 5, 3, 2, 2) and truth["site"][1].tolist() == (6, 4, 3, 2, 5)
    assert truth["site"][2].tolist() == (0, 0, 0, 0, NO_FOUNDER)
    # the same founders across two root populations: the tie is between ids, not hap indices
    rows = [[(10, 30, 1, 1)], [(10, 30, 3, 0)], [(10, 30, 1, 1)], [(10, 30, 3, 0)]]
    truth = check(gpu_lib, rows, [15], [4, 2])
    assert truth["site"][0].tolist() == (8, 4, 2, 2, 3)


def test_a_row_of_five_hundred_parts(gpu_lib):
    """labels cycle through seven founders of two root populations, every 50th part leaves a gap; a one-part row beside it"""
    long_row = [(1000 + 7 * q, 1000 + 7 * (q + 1) - (3 if q % 50 == 49 else 0), q % 7 % 4, q % 7 // 4) for q in range(500)]
    rows = [long_row, [(1003, 1000 + 7 * 480 + 2, 1, 0)]]
    truth = check(gpu_lib, rows, LI.boundary_positions(rows, extra=[0, 999, 5000]), [4, 3])
    assert (truth["site"]["n_covered"] == 2).any() and (truth["site"]["top_count"] == 2).any() and (truth["site"]["n_covered"] == 0).any()


def test_no_positions_and_no_rows(gpu_lib):
    """n_pos == 0 touches nothing; n_rows == 0 writes zeros and a zeroed site with top_founder = NO_FOUNDER, and nothing into fid"""
    f = gpu_lib._f("dbg_lineage_host")
    parts, off = T.lists_of([[[10, 20, 1, 0]]])
    nfh = np.array([2, 3], dtype=np.uint64); pos = np.array([12, 15], dtype=np.uint64)
    fid = np.full((2, 1), 7, dtype=np.uint32); counts = np.full((2, 5), 7, dtype=np.uint32); site = np.zeros(2, dtype=LINEAGE_SITE_DTYPE); pc = np.full((2, 2), 7, dtype=np.uint32)
    site["n_covered"] = 7
    assert f(parts, off, 1, pos, 0, nfh, 2, fid, counts, site, pc) == 0
    assert (fid == 7).all() and (counts == 7).all() and (site["n_covered"] == 7).all() and (pc == 7).all()
    assert f(parts, off, 1, None, 0, nfh, 2, fid, counts, site, pc) == 0 and (counts == 7).all()
    assert f(None, None, 0, pos, 2, nfh, 2, fid, counts, site, pc) == 0
    assert (fid == 7).all() and not counts.any() and not pc.any()
    assert [s.tolist() for s in site] == [(0, 0, 0, 0, NO_FOUNDER)] * 2
    LI.same((None, counts, site, pc), LI.truth([], [12, 15], [2, 3]), "no rows")


def test_each_output_null_in_turn(gpu_lib):
    rs = np.random.RandomState(3)
    rows = [[tuple(q) for q in row] for row in T.random_rows(rs, 9, span=5000, max_parts=8)]
    pos = LI.boundary_positions(rows)[::3]
    for skip in LI.OUTPUTS:
        check(gpu_lib, rows, pos, [6, 6], want=tuple(k for k in LI.OUTPUTS if k != skip))
    for only in LI.OUTPUTS:
        check(gpu_lib, rows, pos, [6, 6], want=(only,))
    assert gpu_lib.dbg_lineage_host(*T.lists_of(rows), pos, [6, 6], want=()) == (None, None, None, None)


def test_random_rows_at_every_boundary(gpu_lib):
    """64 rows with gaps, every part boundary and its two neighbours; a larger founder count than the labels need moves the ids of the
    second root population and nothing else"""
    rs = np.random.RandomState(17)
    rows = [[tuple(q) for q in row] for row in T.random_rows(rs, 64, max_parts=24)]
    pos = LI.boundary_positions(rows, extra=[0, 999, 200_000])
    truth = check(gpu_lib, rows, pos, [6, 6])
    site = truth["site"]
    assert len(pos) > 2000 and (truth["fid"] == NO_FOUNDER).any() and (site["n_covered"] < 64).any() and (site["n_covered"] == 64).any()
    assert (site["n_covered"][:2] == 0).all() and site["n_covered"][-1] == 0
    # the identities
    assert np.array_equal(truth["counts"].sum(axis=1), site["n_covered"]) and np.array_equal(truth["pop_counts"].sum(axis=1), site["n_covered"])
    assert np.array_equal((truth["counts"] != 0).sum(axis=1), site["n_lineages"]) and np.array_equal(truth["counts"].max(axis=1), site["top_count"])
    assert np.array_equal((truth["counts"].astype(np.uint64) ** 2).sum(axis=1), site["sum_sq"])
    assert (LI.ties(truth["counts"]) >= 2).any() and (LI.ties(truth["counts"]) == 1).any()
    wide = check(gpu_lib, rows, pos[::7], [9, 40], want=("fid", "site", "pop_counts"))
    narrow = LI.truth(rows, pos[::7], [6, 6])
    moved = np.where((narrow["fid"] >= 6) & (narrow["fid"] != NO_FOUNDER), narrow["fid"] + 3, narrow["fid"])
    assert np.array_equal(wide["fid"], moved) and np.array_equal(wide["pop_counts"], narrow["pop_counts"])
    for name in ("sum_sq", "n_covered", "n_lineages", "top_count"):
        assert np.array_equal(wide["site"][name], narrow["site"][name])


def test_refusals(gpu_lib):
    """each with its code and its whole message, and nothing written"""
    f = gpu_lib._f("dbg_lineage_host")
    parts, off = T.lists_of([[[10, 20, 1, 0], [20, 30, 3, 1]], [[10, 30, 2, 0]]])
    fid = np.full((3, 2), 7, dtype=np.uint32); counts = np.full((3, 8), 7, dtype=np.uint32); site = np.zeros(3, dtype=LINEAGE_SITE_DTYPE); pc = np.full((3, 2), 7, dtype=np.uint32)
    site["top_count"] = 7

    def refused(code, message, pos, nfh, n_pop=2, lists=(parts, off)):
        pos = None if pos is None else np.array(pos, dtype=np.uint64); nfh = None if nfh is None else np.array(nfh, dtype=np.uint64)
        rc = f(lists[0], lists[1], len(lists[1]) - 1, pos, 0 if pos is None else len(pos), nfh, n_pop, fid, counts, site, pc)
        assert (rc, gpu_lib.last_error()) == (code, message)
        assert (fid == 7).all() and (counts == 7).all() and (site["top_count"] == 7).all() and (pc == 7).all()

    refused(-1, "dbg_lineage_host: the positions decrease at index 2 (14 behind 15)", [12, 15, 14], [4, 4])
    refused(-1, "dbg_lineage_host: a part's hap_index is at or beyond the founder haplotypes given for its root population", [12, 14, 15], [4, 3])
    refused(-1, "dbg_lineage_host: a part's hap_index is at or beyond the founder haplotypes given for its root population", [0, 1, 2], [2, 4])      # (no position is covered by it)
    refused(-1, "dbg_lineage_host: a part names a root population outside [0, 1)", [12, 14, 15], [4], n_pop=1)
    neg = T.lists_of([[[10, 20, 1, -1]]])
    refused(-1, "dbg_lineage_host: a part names a root population outside [0, 2)", [12, 14, 15], [4, 4], lists=neg)
    refused(-5, "dbg_lineage_host: more than 2^32 - 2 founder haplotypes in all", [12, 14, 15], [1 << 31, (1 << 31) - 1])
    refused(-5, "dbg_lineage_host: more than 2^32 - 2 founder haplotypes in all", [12, 14, 15], [TOP, 2])
    refused(-1, "dbg_lineage_host: n_founder_haps is null", [12, 14, 15], None)
    rc = f(parts, off, 2, None, 3, np.array([4, 4], dtype=np.uint64), 2, fid, counts, site, pc)
    assert (rc, gpu_lib.last_error()) == (-1, "dbg_lineage_host: null positions")
    # the largest legal total is taken (no position: nothing of F entries is touched)
    assert f(parts, off, 2, None, 0, np.array([1 << 31, (1 << 31) - 2], dtype=np.uint64), 2, fid, None, site, pc) == 0
    assert gpu_lib.dbg_lineage_tile() >= 256 and gpu_lib.dbg_lineage_tile() % 256 == 0


def test_hand_built_immigrants(gpu_lib):
    """chromosome 0 of migrant_inputs.IMMIGRANTS: 12 rows over three root populations, F = 84, every boundary and its neighbours"""
    rows = [parts for parts, _ in M.rows_of(M.IMMIGRANTS, 0)]
    nfh = [M.n_founders(p) for p in range(M.N_POP)]
    pos = LI.boundary_positions(rows)
    assert (len(rows), sum(nfh), len(pos)) == (12, 84, 1560)
    truth = check(gpu_lib, rows, pos, nfh)
    site, tie = truth["site"], LI.ties(truth["counts"])
    covered = site["n_covered"] > 0
    figures = {"uncovered": int((~covered).sum()), "top_counts": sorted(set(site["top_count"][covered].tolist())),
               "n_lineages": (int(site["n_lineages"][covered].min()), int(site["n_lineages"][covered].max())),
               "tied": float((tie[covered] >= 2).mean()), "unique": float((tie[covered] == 1).mean())}
    print("immigrants:", figures)
    assert figures["uncovered"] == 3 and (site["n_covered"][covered] == 12).all(), figures
    assert {2, 3, 4} <= set(figures["top_counts"]), figures
    assert figures["n_lineages"] == (8, 11), figures
    assert figures["tied"] >= 0.4 and figures["unique"] >= 0.4, figures
    assert np.array_equal(truth["counts"].sum(axis=1), site["n_covered"]) and np.array_equal(truth["pop_counts"].sum(axis=1), site["n_covered"])
    assert (truth["pop_counts"][covered] > 0).all(axis=1).any(), "a position with all three root populations"


def test_reductions_against_fractions():
    """lineage.py: one float64 division of exact integers, NaN where the denominator is 0; labels() splits the ids again"""
    site = np.zeros(7, dtype=LINEAGE_SITE_DTYPE)
    site["n_covered"] = [0, 1, 2, 12, 320, 200_000, (1 << 32) - 1]
    site["sum_sq"] = [0, 1, 2, 30, 1234, 200_000 + 2 * 77, ((1 << 32) - 1) ** 2]
    pc = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 4, 3], [100, 20, 200], [1, 199_998, 1], [(1 << 32) - 1, 0, 0]], dtype=np.uint32)
    fge, pibd, freq = lineage.founder_genome_equivalents(site), lineage.ibd_probability(site), lineage.ancestry_frequency(site, pc)
    assert fge.dtype == pibd.dtype == freq.dtype == np.float64 and freq.shape == (7, 3)
    tol = Fraction(1, 10 ** 15)
    for k in range(7):
        w = LI.fge_fraction(site[k])
        assert math.isnan(fge[k]) if w is None else abs(Fraction(float(fge[k])) - w) <= w * tol, k
        w = LI.ibd_fraction(site[k])
        assert math.isnan(pibd[k]) if w is None else abs(Fraction(float(pibd[k])) - w) <= w * tol, k
        n = int(site["n_covered"][k])
        for q in range(3):
            assert math.isnan(freq[k, q]) if n == 0 else abs(Fraction(float(freq[k, q])) - Fraction(int(pc[k, q]), n)) <= Fraction(int(pc[k, q]), n) * tol, (k, q)
    assert pibd[2] == 0.0 and pibd[6] == 1.0 and fge[6] == 1.0
    rp, hap = lineage.labels(np.array([[0, 3, 4, 9], [10, 12, NO_FOUNDER, 4]], dtype=np.uint32), [4, 0, 6, 3])
    assert rp.dtype == np.int32 and hap.dtype == np.uint64
    assert rp.tolist() == [[0, 0, 2, 2], [3, 3, -1, 2]] and hap.tolist() == [[0, 3, 0, 5], [0, 2, (1 << 64) - 1, 0]]


def test_binding_defaults():
    """the wrapper remembers the founder haplotypes its uploads and syntheses named, per root population, and raises when it knows none"""
    class Ctx(capi.GevContext):
        def __init__(self, n_pop):
            self.n_pop, self._founder_haps, self.h = n_pop, {}, None
    c = Ctx(2)
    with pytest.raises(ValueError, match=r"root population\(s\) \[0, 1\]"):
        c.founder_haps()
    c._saw_founders(0, 28); c._saw_founders(0, 24)
    with pytest.raises(ValueError, match=r"root population\(s\) \[1\]"):
        c.founder_haps()
    c._saw_founders(1, 6)
    assert c.founder_haps().tolist() == [28, 6] and c.founder_haps().dtype == np.uint64
    assert c.founder_haps([3, 4]).tolist() == [3, 4]
    with pytest.raises(AssertionError):
        c.founder_haps([3, 4, 5])
