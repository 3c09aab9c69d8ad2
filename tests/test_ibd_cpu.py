"""gev_dbg_ibd_host: the two-cursor IBD walk of geneevolve_amd/csrc/gev_ibd.h compiled for the host, against the per-position raster of
tests/ibd_inputs.py on constructed lists and on seeded random rows; the reductions of geneevolve_amd/ibd.py against exact fractions.
No device is needed."""
from fractions import Fraction

import numpy as np
import pytest

from geneevolve_amd import ibd
from tests import ibd_inputs as T

BIG = 1 << 63


def check(gpu_lib, rows_a, rows_b=None, min_bp=0):
    """the host build on the lists against the raster, all three outputs -> them"""
    pa, oa = T.lists_of(rows_a)
    pb, ob = (None, None) if rows_b is None else T.lists_of(rows_b)
    got = gpu_lib.dbg_ibd_host(pa, oa, pb, ob, min_bp)
    want = T.truth(pa, oa, pb, ob, min_bp)
    for g, w, name in zip(got, want, ("shared_bp", "n_seg", "max_seg")):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{name}: {g.tolist()} vs {w.tolist()}"
    return [x.tolist() for x in got]


CASES = {
    # name: (rows a, rows b, expected (shared, n_seg, max_seg) of pair (0, 0) or None)
    "a row without parts": ([[]], [[[10, 50, 3, 0]]], (0, 0, 0)),
    "both rows without parts": ([[]], [[]], (0, 0, 0)),
    "a gap inside a row": ([[[10, 20, 3, 0], [30, 50, 3, 0]]], [[[10, 50, 3, 0]]], (30, 2, 20)),
    "adjacent parts of one row with the same label": ([[[10, 20, 3, 0], [20, 50, 3, 0]]], [[[10, 50, 3, 0]]], (40, 1, 40)),
    "both rows change to another common founder together": ([[[10, 20, 3, 0], [20, 50, 4, 0]]], [[[10, 20, 3, 0], [20, 50, 4, 0]]], (40, 1, 40)),
    "both rows change together to different founders": ([[[10, 20, 3, 0], [20, 50, 4, 0]]], [[[10, 20, 3, 0], [20, 50, 5, 0]]], (10, 1, 10)),
    "touching parts with different labels": ([[[10, 20, 3, 0], [20, 50, 4, 0]]], [[[10, 50, 4, 0]]], (30, 1, 30)),
    "equal hap_index under different root populations": ([[[10, 50, 3, 0]]], [[[10, 50, 3, 1]]], (0, 0, 0)),
    "one-bp parts": ([[[10, 11, 1, 0], [11, 12, 1, 0], [12, 13, 2, 0], [13, 14, 1, 0]]], [[[9, 14, 1, 0]]], (3, 2, 2)),
    "positions near 2^63": ([[[BIG - 7, BIG - 1, 1, 0], [BIG - 1, BIG + 9, 2, 0], [BIG + 9, 2 * BIG - 1, 1, 0]]],
                            [[[BIG - 9, BIG + 3, 2, 0], [BIG + 3, 2 * BIG - 2, 1, 0]]], (4 + BIG - 11, 2, BIG - 11)),
    "a hap_index beyond 2^32": ([[[10, 50, (1 << 40) + 3, 0]]], [[[10, 30, 3, 0], [30, 50, (1 << 40) + 3, 0]]], (20, 1, 20)),
    "an overlap on one side of a mismatch only": ([[[0, 100, 1, 0]]], [[[0, 10, 1, 0], [10, 20, 2, 0], [20, 100, 1, 0]]], (90, 2, 80)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_lists(gpu_lib, name):
    rows_a, rows_b, expect = CASES[name]
    got = check(gpu_lib, rows_a, rows_b)
    assert tuple(g[0][0] for g in got) == expect, name
    swapped = check(gpu_lib, rows_b, rows_a)
    assert swapped == got, "the pair the other way round"


def test_one_part_against_five_hundred(gpu_lib):
    """a 1-part row against a 500-part row whose labels cycle through three founders, the one of the short row among them; every 50th
    boundary keeps its label, so that segments of two parts occur"""
    long_row, h = [], 0
    for q in range(500):
        h = h if q % 50 == 49 else (h + 1) % 3
        long_row.append([1000 + 7 * q, 1000 + 7 * (q + 1), h, 0])
    got = check(gpu_lib, [[[1003, 1000 + 7 * 480 + 2, 1, 0]]], [long_row])
    assert got[1][0][0] > 100 and got[2][0][0] == 14


def test_rectangular_and_min_bp(gpu_lib):
    """n_a != n_b; min_bp equal to a segment's length counts it, one more does not; each output NULL in turn"""
    rs = np.random.RandomState(11)
    rows_a, rows_b = T.random_rows(rs, 5), T.random_rows(rs, 9)
    got = check(gpu_lib, rows_a, rows_b)
    assert np.shape(got[0]) == (5, 9)
    pa, oa = T.lists_of(rows_a); pb, ob = T.lists_of(rows_b)
    segs = T.all_segments(pa, oa, pb, ob)
    a, b = next((a, b) for a in range(5) for b in range(9) if len(set(segs[a][b])) >= 2)
    length = sorted(set(segs[a][b]))[1]
    at = check(gpu_lib, rows_a, rows_b, min_bp=length)
    above = check(gpu_lib, rows_a, rows_b, min_bp=length + 1)
    n_at = sum(1 for x in segs[a][b] if x == length)
    assert at[1][a][b] - above[1][a][b] == n_at >= 1 and at[0][a][b] - above[0][a][b] == n_at * length
    assert check(gpu_lib, rows_a, rows_b, min_bp=(1 << 64) - 1)[1] == np.zeros((5, 9), dtype=int).tolist()
    want = T.truth(pa, oa, pb, ob, 0, segs)
    for skip in range(3):
        flags = tuple(k != skip for k in range(3))
        outs = gpu_lib.dbg_ibd_host(pa, oa, pb, ob, 0, want=flags)
        assert outs[skip] is None and all(np.array_equal(o, w) for o, w in zip(outs, want) if o is not None)
    assert gpu_lib.dbg_ibd_host(pa, oa, pb, ob, 0, want=(False, False, False)) == (None, None, None)
    empty = gpu_lib.dbg_ibd_host(pa, oa[:1], pb, ob)
    assert empty[0].shape == (0, 9)


def test_random_rows_all_pairs(gpu_lib):
    """60 rows of 1 to 40 parts over 12 labels, all pairs; the matrix is symmetric and a row shares its covered length with itself"""
    rs = np.random.RandomState(20240)
    rows = T.random_rows(rs, 60)
    pa, oa = T.lists_of(rows)
    segs = T.all_segments(pa, oa)
    got = gpu_lib.dbg_ibd_host(pa, oa)
    for min_bp in (0, 2500):
        got = gpu_lib.dbg_ibd_host(pa, oa, min_bp=min_bp)
        want = T.truth(pa, oa, min_bp=min_bp, seg_lists=segs)
        for g, w, name in zip(got, want, ("shared_bp", "n_seg", "max_seg")):
            assert np.array_equal(g, w), f"{name}, min_bp {min_bp}: {np.argwhere(g != w)[:5].tolist()}"
            assert np.array_equal(g, g.T)
    sh, ns, _ = gpu_lib.dbg_ibd_host(pa, oa)
    covered = [sum(en - st for st, en, _, _ in r) for r in rows]
    assert np.array_equal(np.diag(sh), covered)
    off_diag = ns[~np.eye(60, dtype=bool)]
    assert (off_diag == 0).any() and (off_diag >= 2).any(), "the inputs were meant to hold pairs that share nothing and pairs with several segments"
    assert T.adjacent_same_label(pa, oa) > 0


def test_host_refusals(gpu_lib):
    pa, oa = T.lists_of([[[1, 5, 0, 0]]])
    f = gpu_lib._f("dbg_ibd_host")
    sh = np.full((1, 1), 7, dtype=np.uint64)
    assert f(pa, None, 1, pa, oa, 1, 0, sh, None, None) == -1 and "offsets" in gpu_lib.last_error() and sh[0, 0] == 7
    assert f(None, oa, 1, pa, oa, 1, 0, sh, None, None) == -1 and "parts" in gpu_lib.last_error() and sh[0, 0] == 7
    assert f(pa, oa[::-1].copy(), 1, pa, oa, 1, 0, sh, None, None) == -1 and "decrease" in gpu_lib.last_error() and sh[0, 0] == 7
    assert f(None, None, 0, None, None, 0, 0, None, None, None) == 0


def test_reductions_against_fractions():
    """coancestry, inbreeding and admixture from integer sums: each entry one float64 division of exact integers"""
    rs = np.random.RandomState(5)
    n, span = 7, 3 * 123_456_789
    s = rs.randint(0, span + 1, size=(2 * n, 2 * n)).astype(np.uint64)
    s = np.maximum(s, s.T)
    got = ibd.coancestry_from_sums(s, span)
    want = T.coancestry_fractions(s, span)
    for i in range(n):
        for k in range(n):
            assert abs(Fraction(float(got[i, k])) - want[i][k]) <= want[i][k] * Fraction(1, 10 ** 15)
    own = s[np.arange(0, 2 * n, 2), np.arange(1, 2 * n, 2)]
    f = ibd.inbreeding_from_sums(own, span)
    for i in range(n):
        w = Fraction(int(own[i]), span)
        assert abs(Fraction(float(f[i])) - w) <= w * Fraction(1, 10 ** 15)
    bp = rs.randint(0, 10 ** 9, size=(2 * n, 3)).astype(np.uint64)
    bp[4:6] = 0                                                  # an individual whose rows cover nothing
    adm = ibd.admixture_from_sums(bp)
    assert np.isnan(adm[2]).all()
    for i in (0, 1, 3, 4, 5, 6):
        tot = int(bp[2 * i].sum() + bp[2 * i + 1].sum())
        for p in range(3):
            w = Fraction(int(bp[2 * i, p]) + int(bp[2 * i + 1, p]), tot)
            assert abs(Fraction(float(adm[i, p])) - w) <= w * Fraction(1, 10 ** 15)
        assert abs(adm[i].sum() - 1.0) < 1e-15 * 4
