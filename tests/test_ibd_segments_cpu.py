"""gev_dbg_ibd_segments_host: the IBD segment list by the walk of geneevolve_amd/csrc/gev_ibd.h compiled for the host, against the runs
of the raster (tests/ibd_segments_inputs.py) on the constructed lists of test_ibd_cpu.py and on seeded random rows; thresholds, the
capacity rule, consistency with gev_dbg_ibd_host, the refusals, and the list helpers of geneevolve_amd/ibd.py.  Every comparison is
equality.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from geneevolve_amd import capi, ibd
from geneevolve_amd.capi import SEGMENT_DTYPE
from tests import ibd_inputs as T
from tests import ibd_segments_inputs as S
from tests.test_ibd_cpu import CASES

SENTINEL = S.SENTINEL


def test_record_layout():
    assert SEGMENT_DTYPE.itemsize == 24 and SEGMENT_DTYPE.names == ("st", "en", "row_a", "row_b")
    assert [SEGMENT_DTYPE.fields[n][1] for n in SEGMENT_DTYPE.names] == [0, 8, 16, 20]


def check(gpu_lib, rows_a, rows_b, min_bp=0):
    pa, oa = T.lists_of(rows_a); pb, ob = T.lists_of(rows_b)
    got = gpu_lib.dbg_ibd_segments_host(pa, oa, pb, ob, min_bp)
    S.same(got, S.records(S.all_runs(pa, oa, pb, ob), min_bp), "host build against the raster")
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_lists(gpu_lib, name):
    rows_a, rows_b, expect = CASES[name]
    got = check(gpu_lib, rows_a, rows_b)
    assert len(got) == expect[1] and sum(en - st for st, en, _, _ in got.tolist()) == expect[0]
    assert max((en - st for st, en, _, _ in got.tolist()), default=0) == expect[2]
    swapped = check(gpu_lib, rows_b, rows_a)
    back = swapped.copy(); back["row_a"], back["row_b"] = swapped["row_b"], swapped["row_a"]
    S.same(back, got, "the pair the other way round")


def test_one_part_against_five_hundred(gpu_lib):
    long_row, h = [], 0
    for q in range(500):
        h = h if q % 50 == 49 else (h + 1) % 3
        long_row.append([1000 + 7 * q, 1000 + 7 * (q + 1), h, 0])
    short = [[1003, 1000 + 7 * 480 + 2, 1, 0]]
    got = check(gpu_lib, [short], [long_row])
    assert len(got) > 100 and int((got["en"] - got["st"]).max()) == 14
    swapped = check(gpu_lib, [long_row], [short])
    assert np.array_equal(swapped["st"], got["st"]) and np.array_equal(swapped["en"], got["en"])


class Random:
    """60 rows of random_rows and the raster's runs of all their pairs (computed once and left unchanged)"""

    def __init__(self):
        rs = np.random.RandomState(20240)
        self.rows = T.random_rows(rs, 60)
        self.parts, self.off = T.lists_of(self.rows)
        self.runs = S.all_runs(self.parts, self.off)
        self.lengths = sorted({en - st for row in self.runs for r in row for st, en in r})


@pytest.fixture(scope="module")
def rnd():
    return Random()


def min_bps(lengths):
    """0, an occurring length, that plus one, one beyond every segment"""
    exact = lengths[len(lengths) // 2]
    return (0, exact, exact + 1, lengths[-1] + 1)


def test_random_rows_square(gpu_lib, rnd):
    for upper in (False, True):
        for min_bp in min_bps(rnd.lengths):
            got = gpu_lib.dbg_ibd_segments_host(rnd.parts, rnd.off, min_bp=min_bp, upper=upper)
            want = S.records(rnd.runs, min_bp, upper)
            S.same(got, want, f"60 x 60, upper {upper}, min_bp {min_bp}")
            assert (len(got) == 0) == (min_bp > rnd.lengths[-1])
    full = S.records(rnd.runs)
    key = np.lexsort((full["st"], full["row_b"], full["row_a"]))
    assert np.array_equal(key, np.arange(len(full))), "the truth itself is in (row_a, row_b, st) order"
    exact = min_bps(rnd.lengths)[1]
    n_at = len(S.records(rnd.runs, exact)) - len(S.records(rnd.runs, exact + 1))
    assert n_at >= 1, "the length occurs"
    up = S.records(rnd.runs, 0, True)
    assert (up["row_a"] < up["row_b"]).all() and 0 < len(up) < len(full) / 2


def test_random_rows_rectangular(gpu_lib, rnd):
    """rows [0, 23) x [23, 60) as two separate lists, and the prefixes [0, 23) x [0, 60) of one list in both pair modes"""
    cut = int(rnd.off[23])
    pa, oa = rnd.parts[:cut], rnd.off[:24]
    pb, ob = rnd.parts[cut:], rnd.off[23:] - rnd.off[23]
    for min_bp in min_bps(rnd.lengths)[:3]:
        got = gpu_lib.dbg_ibd_segments_host(pa, oa, pb, ob, min_bp)
        S.same(got, S.records(rnd.runs, min_bp, a=(0, 23), b=(23, 37), row_a0=0, row_b0=0), f"23 x 37, min_bp {min_bp}")
    f = gpu_lib._f("dbg_ibd_segments_host")
    for pairs in (capi.IBD_ALL_PAIRS, capi.IBD_UPPER):
        want = S.records(rnd.runs, 0, pairs == capi.IBD_UPPER, a=(0, 23))
        n = C.c_uint64()
        out = np.zeros(len(want), dtype=SEGMENT_DTYPE)
        assert f(rnd.parts, rnd.off, 23, rnd.parts, rnd.off, 60, 0, pairs, out, len(out), C.byref(n)) == 0 and n.value == len(want)
        S.same(out, want, f"23 x 60 of one list, pairs {pairs}")


def test_consistency_with_the_summaries(gpu_lib, rnd):
    for min_bp in min_bps(rnd.lengths)[:3]:
        sh, ns, mx = gpu_lib.dbg_ibd_host(rnd.parts, rnd.off, min_bp=min_bp)
        cnt, tot, longest = S.per_pair(gpu_lib.dbg_ibd_segments_host(rnd.parts, rnd.off, min_bp=min_bp), 60, 60)
        assert cnt == ns.tolist() and tot == [[int(x) for x in r] for r in sh] and longest == [[int(x) for x in r] for r in mx]


def test_capacity(gpu_lib, rnd):
    f = gpu_lib._f("dbg_ibd_segments_host")
    S.capacity_cases(f, (rnd.parts, rnd.off, 60, rnd.parts, rnd.off, 60, 0, capi.IBD_ALL_PAIRS), S.records(rnd.runs))
    S.capacity_cases(f, (rnd.parts, rnd.off, 60, rnd.parts, rnd.off, 60, 2500, capi.IBD_UPPER), S.records(rnd.runs, 2500, True))
    # a threshold beyond every segment: zero records, out untouched
    rc, n, buf = S.raw(f, (rnd.parts, rnd.off, 60, rnd.parts, rnd.off, 60, rnd.lengths[-1] + 1, capi.IBD_ALL_PAIRS), 4)
    assert rc == 0 and n == 0 and (buf == SENTINEL).all()
    for na, nb in ((0, 60), (60, 0), (0, 0)):
        rc, n, buf = S.raw(f, (rnd.parts, rnd.off, na, rnd.parts, rnd.off, nb, 0, capi.IBD_ALL_PAIRS), 4)
        assert rc == 0 and n == 0 and (buf == SENTINEL).all()


def test_host_refusals(gpu_lib):
    pa, oa = T.lists_of([[[1, 5, 0, 0]], [[1, 9, 0, 0]]])
    pb, ob = T.lists_of([[[1, 5, 0, 0]], [[1, 9, 0, 0]]])
    f = gpu_lib._f("dbg_ibd_segments_host")

    def refused(code, word, *args, n_total=True):
        out = np.full(8 * SEGMENT_DTYPE.itemsize, SENTINEL, dtype=np.uint8)
        n = C.c_uint64(12345)
        rc = f(*args, capi._p(out), 8, C.byref(n) if n_total else None)
        assert rc == code and word in gpu_lib.last_error(), f"{rc} {gpu_lib.last_error()}"
        assert (out == SENTINEL).all() and n.value == 12345

    refused(-1, "same lists", pa, oa, 2, pb, ob, 2, 0, capi.IBD_UPPER)
    refused(-1, "offsets", pa, None, 2, pb, ob, 2, 0, capi.IBD_ALL_PAIRS)
    refused(-1, "parts", None, oa, 2, pb, ob, 2, 0, capi.IBD_ALL_PAIRS)
    refused(-1, "decrease", pa, oa[::-1].copy(), 2, pb, ob, 2, 0, capi.IBD_ALL_PAIRS)
    refused(-1, "n_total", pa, oa, 2, pb, ob, 2, 0, capi.IBD_ALL_PAIRS, n_total=False)
    refused(-1, "pairs", pa, oa, 2, pb, ob, 2, 0, 2)
    n = C.c_uint64()
    assert f(pa, oa, 2, pb, ob, 2, 0, 0, None, 3, C.byref(n)) == -1 and "null output" in gpu_lib.last_error()
    assert f(pa, oa, 2, pa, oa, 2, 0, capi.IBD_UPPER, None, 0, C.byref(n)) == 0 and n.value == 1
    assert f(None, None, 0, None, None, 0, 0, 0, None, 0, C.byref(n)) == 0 and n.value == 0


def test_segment_individuals_and_chromosome_order():
    seg = np.zeros(4, dtype=SEGMENT_DTYPE)
    seg["row_a"] = [0, 1, 6, 7]; seg["row_b"] = [9, 8, 3, 2]
    ia, ca, ib, cb = ibd.segment_individuals(seg)
    assert ia.tolist() == [0, 0, 3, 3] and ca.tolist() == [0, 1, 0, 1] and ib.tolist() == [4, 4, 1, 1] and cb.tolist() == [1, 0, 1, 0]
    # two chromosomes' host results, handed over in descending order of chromosome
    rs = np.random.RandomState(3)
    per_chr = []
    lib_rows = [T.random_rows(rs, 6, max_parts=6, n_labels=4) for _ in range(2)]
    for rows in lib_rows:
        p, o = T.lists_of(rows)
        per_chr.append(S.records(S.all_runs(p, o), upper=True))
    assert all(len(x) for x in per_chr)
    both = ibd.segments_over_chromosomes([1, 0], [per_chr[1], per_chr[0]])
    assert both.dtype.names == ("chr", "st", "en", "row_a", "row_b") and both["chr"].dtype == np.int32
    assert both["chr"].tolist() == [0] * len(per_chr[0]) + [1] * len(per_chr[1])
    for k in range(2):
        mine = both[both["chr"] == k]
        assert all(np.array_equal(mine[name], per_chr[k][name]) for name in SEGMENT_DTYPE.names)
    key = np.lexsort((both["st"], both["row_b"], both["row_a"], both["chr"]))
    assert np.array_equal(key, np.arange(len(both)))
    assert len(ibd.segments_over_chromosomes([], [])) == 0
