"""The truth of the IBD segment list tests (test_ibd_segments_cpu.py, test_gpu_ibd_segments.py): the (st, en) runs over the elementary
intervals of ibd_inputs.raster.  Consecutive elementary intervals are merged where both rows are covered and their labels are equal;
the runs are filtered by min_bp and by the pair mode and put in (row_a, row_b, st) order.  Independent of the two-cursor walk of
geneevolve_amd/csrc/gev_ibd.h, as ibd_inputs.truth is."""
import ctypes as C

import numpy as np

from geneevolve_amd.capi import SEGMENT_DTYPE, _p
from tests import ibd_inputs as T


def runs(edges, la, lb):
    """the IBD segments of two label vectors as [(st, en)] of Python integers, in position order"""
    shared = np.zeros(len(la) + 2, dtype=np.int8)                 # per elementary interval: both rows covered, labels equal; a 0 at each end
    shared[1:-1] = (la >= 0) & (la == lb)
    step = np.diff(shared)
    return [(edges[s], edges[e]) for s, e in zip(np.flatnonzero(step == 1).tolist(), np.flatnonzero(step == -1).tolist())]


def all_runs(parts_a, off_a, parts_b=None, off_b=None):
    """[n_a][n_b] lists of (st, en)"""
    edges, la, lb = T.raster(parts_a, off_a, parts_b, off_b)
    return [[runs(edges, la[a], lb[b]) for b in range(len(lb))] for a in range(len(la))]


def records(run_lists, min_bp=0, upper=False, a=None, b=None, row_a0=None, row_b0=None):
    """SEGMENT_DTYPE records of the pairs (i, k), i in range a = (begin, n), k in range b (None: all), of run_lists [n_a][n_b]; the
    records name rows row_a0 + i - a[0], row_b0 + k - b[0] (None: i, k themselves).  upper: only pairs whose named rows have
    row_a < row_b"""
    a = (0, len(run_lists)) if a is None else a
    b = (0, len(run_lists[0]) if run_lists else 0) if b is None else b
    row_a0 = a[0] if row_a0 is None else row_a0
    row_b0 = b[0] if row_b0 is None else row_b0
    out = []
    for i in range(a[0], a[0] + a[1]):
        for k in range(b[0], b[0] + b[1]):
            ra, rb = row_a0 + i - a[0], row_b0 + k - b[0]
            if upper and ra >= rb:
                continue
            out.extend((st, en, ra, rb) for st, en in run_lists[i][k] if en - st >= min_bp)
    rec = np.zeros(len(out), dtype=SEGMENT_DTYPE)
    for col, name in enumerate(SEGMENT_DTYPE.names):
        rec[name] = np.array([r[col] for r in out], dtype=SEGMENT_DTYPE.fields[name][0])
    return rec


def same(got, want, what):
    assert got.dtype == SEGMENT_DTYPE and got.shape == want.shape, f"{what}: {got.dtype}{got.shape}, expected {want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)[:3]
        raise AssertionError(f"{what}: differs at {bad.tolist()}: {got[bad].tolist()} vs {want[bad].tolist()}")


SENTINEL = 0xA5


def raw(f, args, capacity, guard=3):
    """one raw call f(*args, out, capacity, &n_total) on a sentinel-filled buffer of capacity + guard records (out is NULL with
    capacity 0) -> (rc, n_total, the buffer's bytes)"""
    buf = np.full((capacity + guard) * SEGMENT_DTYPE.itemsize, SENTINEL, dtype=np.uint8)
    n = C.c_uint64(12345)
    rc = f(*args, _p(buf) if capacity else None, capacity, C.byref(n))
    return rc, n.value, buf


def capacity_cases(f, args, want):
    """count-only, capacity == n_total, one short, two to spare: what lies at or beyond out[capacity] is never written"""
    size = SEGMENT_DTYPE.itemsize
    assert len(want) >= 2
    rc, n, buf = raw(f, args, 0)
    assert rc == 0 and n == len(want) and (buf == SENTINEL).all()
    rc, n, buf = raw(f, args, len(want))
    assert rc == 0 and n == len(want) and buf[:n * size].tobytes() == want.tobytes() and (buf[n * size:] == SENTINEL).all()
    rc, n, buf = raw(f, args, len(want) - 1)
    assert rc == 0 and n == len(want) and (buf == SENTINEL).all(), "one short: the total is right and nothing is written"
    rc, n, buf = raw(f, args, len(want) + 2)
    assert rc == 0 and n == len(want) and buf[:n * size].tobytes() == want.tobytes() and (buf[n * size:] == SENTINEL).all()


def per_pair(rec, n_a, n_b, row_a0=0, row_b0=0):
    """(count, summed length, longest) [n_a][n_b] of records, in Python integers"""
    cnt = [[0] * n_b for _ in range(n_a)]; tot = [[0] * n_b for _ in range(n_a)]; mx = [[0] * n_b for _ in range(n_a)]
    for st, en, ra, rb in rec.tolist():
        i, k, length = ra - row_a0, rb - row_b0, en - st
        cnt[i][k] += 1; tot[i][k] += length; mx[i][k] = max(mx[i][k], length)
    return cnt, tot, mx
