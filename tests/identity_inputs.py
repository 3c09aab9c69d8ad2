"""The truth of the identity-state tests (test_identity_cpu.py, test_gpu_identity.py).  It takes the labels of every row on the elementary
intervals from the raster of tests/ibd_inputs.py, writes the four labels of a pair of individuals as a restricted-growth string and looks
that string up in a literal table of the 15 partitions of four haplotypes.  No cursor and none of the comparisons of
geneevolve_amd/csrc/gev_identity.h: the classification is stated twice, independently.  Python integers throughout."""
from fractions import Fraction

import numpy as np

from tests import ibd_inputs as T

# restricted-growth string of (a0, a1, b0, b1) -> Jacquard's condensed identity state (1 .. 9)
STATE_OF = {
    "0000": 1,
    "0011": 2,
    "0001": 3, "0010": 3,
    "0012": 4,
    "0100": 5, "0111": 5,
    "0122": 6,
    "0101": 7, "0110": 7,
    "0102": 8, "0120": 8, "0112": 8, "0121": 8,
    "0123": 9,
}
assert len(STATE_OF) == 15
SWAPPED = {1: 1, 2: 2, 3: 5, 4: 6, 5: 3, 6: 4, 7: 7, 8: 8, 9: 9}      # the state of (b, a) from that of (a, b)


def growth_string(labels):
    """'0102' for labels (x, y, x, z): every label by the order of its first appearance"""
    seen = []
    for x in labels:
        if x not in seen:
            seen.append(x)
    return "".join(str(seen.index(x)) for x in labels)


def pair_partitions(edges, la, lb, i, k):
    """{restricted-growth string: base pairs} of individual i of side a against individual k of side b, over the elementary intervals
    on which all four rows are covered"""
    return _pair_partitions(_widths(edges), la, lb, i, k)


def _widths(edges):
    """the lengths of the elementary intervals as uint64 (each is below 2^64, and so is every sum of them: they are disjoint)"""
    return np.array([edges[e + 1] - edges[e] for e in range(len(edges) - 1)], dtype=np.uint64)


def _pair_partitions(widths, la, lb, i, k):
    """the elementary intervals are first grouped by their four labels (so that the string is made once per distinct quadruple, not
    once per interval: the fixtures have thousands of intervals and dozens of quadruples); the lengths of a group are added in uint64,
    which is exact here, and are Python integers from there on"""
    four = np.stack([la[2 * i], la[2 * i + 1], lb[2 * k], lb[2 * k + 1]], axis=1)
    covered = (four >= 0).all(axis=1)
    if not covered.any():
        return {}
    quads, group = np.unique(four[covered], axis=0, return_inverse=True)
    sums = np.zeros(len(quads), dtype=np.uint64)
    np.add.at(sums, group.ravel(), widths[covered])
    out = {}
    for quad, bp in zip(quads.tolist(), sums.tolist()):
        s = growth_string(quad)
        out[s] = out.get(s, 0) + int(bp)
    return out


def all_partitions(parts_a, off_a, parts_b=None, off_b=None):
    """[n_a][n_b] dictionaries of pair_partitions"""
    edges, la, lb = T.raster(parts_a, off_a, parts_b, off_b)
    assert len(la) % 2 == 0 and len(lb) % 2 == 0
    widths = _widths(edges)
    return [[_pair_partitions(widths, la, lb, i, k) for k in range(len(lb) // 2)] for i in range(len(la) // 2)]


def truth(parts_a, off_a, parts_b=None, off_b=None, partitions=None):
    """uint64 [9][n_a][n_b] from the raster; partitions: the result of all_partitions, to share it"""
    P = all_partitions(parts_a, off_a, parts_b, off_b) if partitions is None else partitions
    n_a, n_b = len(P), len(P[0]) if P else (len(off_a if off_b is None else off_b) - 1) // 2
    D = np.zeros((9, n_a, n_b), dtype=np.uint64)
    for i in range(n_a):
        for k in range(n_b):
            sums = [0] * 9
            for s, bp in P[i][k].items():
                sums[STATE_OF[s] - 1] += bp
            for q in range(9):
                D[q, i, k] = sums[q]
    return D


def transposed(D):
    """what the call gives with the sides swapped: the planes permuted by SWAPPED, each transposed"""
    return np.stack([D[SWAPPED[s + 1] - 1].T for s in range(9)])


def individuals_of(rows_per_individual):
    """[(row a0, row a1), ...] of [st, en, hap_index, root_pop] lists -> (parts, offsets) with 2 n + 1 offsets"""
    return T.lists_of([r for pair in rows_per_individual for r in pair])


def fractions_of(D, i, k):
    """the statistics of geneevolve_amd/identity.py for one pair as exact Fractions (None where the planes sum to 0):
    {"jacquard": [9], "kinship", "k0", "k1", "k2", "f_a", "f_b"}"""
    d = [int(D[q][i][k]) for q in range(9)]
    tot = sum(d)
    if tot == 0:
        return None
    return {"jacquard": [Fraction(x, tot) for x in d],
            "kinship": Fraction(4 * d[0] + 2 * (d[2] + d[4] + d[6]) + d[7], 4 * tot),
            "k0": Fraction(d[1] + d[3] + d[5] + d[8], tot), "k1": Fraction(d[2] + d[4] + d[7], tot), "k2": Fraction(d[0] + d[6], tot),
            "f_a": Fraction(d[0] + d[1] + d[2] + d[3], tot), "f_b": Fraction(d[0] + d[1] + d[4] + d[5], tot)}
