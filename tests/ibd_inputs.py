"""Inputs and the truth of the IBD tests (test_ibd_cpu.py, test_gpu_ibd.py).  The truth is a raster, independent of the two-cursor walk
of geneevolve_amd/csrc/gev_ibd.h: the labels of every row on the elementary intervals (the sorted union of all part boundaries), rows
compared pointwise by equality, run lengths taken over consecutive equal elementary intervals."""
from fractions import Fraction

import numpy as np

from geneevolve_amd.capi import PART_DTYPE


def parts_of(rows):
    """[st, en, hap_index, root_pop] rows (Python integers of any size below 2^64) -> gev_part records"""
    p = np.zeros(len(rows), dtype=PART_DTYPE)
    for q, (st, en, h, rp) in enumerate(rows):
        p[q] = (st, en, h, rp, 0)
    return p


def lists_of(rows_of_rows):
    """one list of [st, en, hap_index, root_pop] rows per haplotype row -> (parts, offsets) as download_intervals returns them"""
    off = np.zeros(len(rows_of_rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows_of_rows], dtype=np.uint64)
    return parts_of([x for r in rows_of_rows for x in r]), off


def raster(parts_a, off_a, parts_b=None, off_b=None):
    """-> (edges, lab_a, lab_b): edges = the sorted boundaries of all parts of both sides (Python integers); lab_*[r][e] = the label id
    (an integer per distinct (root_population, hap_index), -1 = not covered) of row r on the elementary interval [edges[e], edges[e+1])"""
    sides = [(parts_a, off_a)] + ([(parts_b, off_b)] if parts_b is not None else [])
    bounds = set()
    for parts, _ in sides:
        bounds.update(int(x) for x in parts["st"]); bounds.update(int(x) for x in parts["en"])
    edges = sorted(bounds)
    at = {x: e for e, x in enumerate(edges)}
    ids = {}
    labs = []
    for parts, off in sides:
        lab = np.full((len(off) - 1, max(len(edges) - 1, 0)), -1, dtype=np.int64)
        for r in range(len(off) - 1):
            for q in range(int(off[r]), int(off[r + 1])):
                st, en = int(parts["st"][q]), int(parts["en"][q])
                if en <= st:
                    continue
                key = (int(parts["root_population"][q]), int(parts["hap_index"][q]))
                e0, e1 = at[st], at[en]
                assert (lab[r, e0:e1] == -1).all(), "the parts of a row must not overlap"
                lab[r, e0:e1] = ids.setdefault(key, len(ids))
        labs.append(lab)
    return edges, labs[0], labs[-1]


def segments(edges, la, lb):
    """the IBD segments of two label vectors as a list of lengths (Python integers), in position order"""
    out, run = [], 0
    for e in range(len(edges) - 1):
        if la[e] >= 0 and la[e] == lb[e]:
            run += edges[e + 1] - edges[e]
        elif run:
            out.append(run); run = 0
    if run:
        out.append(run)
    return out


def truth(parts_a, off_a, parts_b=None, off_b=None, min_bp=0, seg_lists=None):
    """(shared_bp uint64, n_seg uint32, max_seg uint64) [n_a][n_b] from the raster; seg_lists: the result of all_segments, to share it"""
    segs = all_segments(parts_a, off_a, parts_b, off_b) if seg_lists is None else seg_lists
    n_a, n_b = len(segs), len(segs[0]) if segs else 0
    sh = np.zeros((n_a, n_b), dtype=np.uint64); ns = np.zeros((n_a, n_b), dtype=np.uint32); mx = np.zeros((n_a, n_b), dtype=np.uint64)
    for a in range(n_a):
        for b in range(n_b):
            s = [x for x in segs[a][b] if x >= min_bp]
            sh[a, b], ns[a, b], mx[a, b] = sum(s), len(s), max(s, default=0)
    return sh, ns, mx


def all_segments(parts_a, off_a, parts_b=None, off_b=None):
    """[n_a][n_b] lists of segment lengths"""
    edges, la, lb = raster(parts_a, off_a, parts_b, off_b)
    return [[segments(edges, la[a], lb[b]) for b in range(len(lb))] for a in range(len(la))]


def adjacent_same_label(parts, off):
    """adjacent parts inside a row that touch and carry the same label"""
    n = 0
    for r in range(len(off) - 1):
        for q in range(int(off[r]), int(off[r + 1]) - 1):
            p, nx = parts[q], parts[q + 1]
            n += int(p["en"] == nx["st"] and p["hap_index"] == nx["hap_index"] and p["root_population"] == nx["root_population"])
    return n


def random_rows(rs, n_rows, span=100_000, max_parts=40, n_labels=12):
    """rows of 1 to max_parts parts over n_labels labels (two root populations) that tile [1000, 1000 + span), with now and then a gap"""
    labels = [(int(h), int(rp)) for rp in range(2) for h in range(n_labels // 2)]
    rows = []
    for _ in range(n_rows):
        k = int(rs.randint(1, max_parts + 1))
        cuts = [1000] + sorted(int(x) for x in rs.choice(np.arange(1001, 1000 + span), k - 1, replace=False)) + [1000 + span]
        row = []
        for q in range(k):
            h, rp = labels[int(rs.randint(len(labels)))]
            st, en = cuts[q], cuts[q + 1]
            if rs.rand() < 0.1 and en - st > 2:
                en -= int(rs.randint(1, en - st))                 # a gap behind this part
            row.append([st, en, h, rp])
        rows.append(row)
    return rows


def coancestry_fractions(shared_sum, span_sum):
    """[n][n] Fractions from the [2 n][2 n] integer sums"""
    n = len(shared_sum) // 2
    return [[Fraction(sum(int(shared_sum[2 * i + x][2 * k + y]) for x in range(2) for y in range(2)), 4 * int(span_sum)) for k in range(n)] for i in range(n)]
