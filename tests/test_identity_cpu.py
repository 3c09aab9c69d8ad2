"""gev_dbg_identity_host: the four-cursor walk of geneevolve_amd/csrc/gev_identity.h compiled for the host, against the table lookup of
tests/identity_inputs.py on constructed lists (each of the 15 partitions of four haplotypes by name, the edge cases of the lists) and on
seeded random individuals; the transpose identity; the refusals; the statistics of geneevolve_amd/identity.py against exact fractions.
No device is needed."""
from fractions import Fraction

import numpy as np
import pytest

from geneevolve_amd import identity
from tests import ibd_inputs as T
from tests import identity_inputs as J

BIG = 1 << 63
FAR = (1 << 40) + 3                                     # a hap_index beyond 2^32 whose low word is another label's


def check(gpu_lib, ind_a, ind_b=None):
    """the host build on the individuals' lists against the table lookup, and the other way round -> [9][n_a][n_b] as lists"""
    pa, oa = J.individuals_of(ind_a)
    pb, ob = (None, None) if ind_b is None else J.individuals_of(ind_b)
    got = gpu_lib.dbg_identity_host(pa, oa, pb, ob)
    want = J.truth(pa, oa, pb, ob)
    assert got.dtype == np.uint64 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), f"{got.tolist()} vs {want.tolist()}"
    if ind_b is not None:
        assert np.array_equal(gpu_lib.dbg_identity_host(pb, ob, pa, oa), J.transposed(got)), "the pair the other way round"
    return got.tolist()


def planes(**states):
    """the nine sums of one pair from d1=..., d7=...; the others 0"""
    return [states.get(f"d{s}", 0) for s in range(1, 10)]


def rows_of_string(s, st, en):
    """four one-part rows on [st, en) whose labels follow the restricted-growth string: digit d -> hap_index 10 + d"""
    return [[[st, en, 10 + int(d), 0]] for d in s]


@pytest.mark.parametrize("string", sorted(J.STATE_OF))
def test_each_partition_by_name(gpu_lib, string):
    """four rows of one part whose labels form the partition: its width lands in the plane the table names and nowhere else"""
    r = rows_of_string(string, 100, 137)
    got = check(gpu_lib, [(r[0], r[1])], [(r[2], r[3])])
    assert [g[0][0] for g in got] == planes(**{f"d{J.STATE_OF[string]}": 37}), string


def test_all_partitions_along_one_pair(gpu_lib):
    """the 15 partitions one behind the other on one pair of individuals, each with a width of its own"""
    rows, want, at = [[], [], [], []], [0] * 9, 1000
    for q, s in enumerate(sorted(J.STATE_OF)):
        w = 3 * q + 1
        for h, r in enumerate(rows_of_string(s, at, at + w)):
            rows[h] += r
        want[J.STATE_OF[s] - 1] += w
        at += w
    got = check(gpu_lib, [(rows[0], rows[1])], [(rows[2], rows[3])])
    assert [g[0][0] for g in got] == want and all(want)


ONE = [[10, 50, 1, 0]]
CASES = {
    # name: ((a0, a1), (b0, b1), the nine sums)
    "a gap in one of the four rows": (([[10, 20, 1, 0], [30, 50, 1, 0]], ONE), (ONE, ONE), planes(d1=30)),
    "a row without parts": ((ONE, []), (ONE, ONE), planes()),
    "all four rows without parts": (([], []), ([], []), planes()),
    "zero-length and inverted parts": (([[10, 10, 9, 0], [10, 30, 1, 0], [30, 30, 9, 0], [35, 32, 9, 0], [35, 50, 1, 0]], ONE), (ONE, [[10, 10, 9, 0], [10, 50, 1, 0], [50, 50, 9, 0]]), planes(d1=35)),
    "adjacent same-label parts": (([[10, 20, 1, 0], [20, 50, 1, 0]], ONE), (ONE, [[10, 30, 1, 0], [30, 50, 1, 0]]), planes(d1=40)),
    "a common change of founder": (([[10, 20, 1, 0], [20, 50, 2, 0]],) * 2, ([[10, 20, 1, 0], [20, 50, 2, 0]],) * 2, planes(d1=40)),
    "a change of founder on side a alone": (([[10, 20, 1, 0], [20, 50, 2, 0]],) * 2, (ONE, ONE), planes(d1=10, d2=30)),
    "equal hap_index under two root populations": (([[10, 50, 3, 0]],) * 2, ([[10, 50, 3, 1]],) * 2, planes(d2=40)),
    "one-bp parts": (([[10, 11, 1, 0], [11, 12, 2, 0], [12, 13, 1, 0], [13, 14, 2, 0]], [[10, 14, 1, 0]]), ([[10, 14, 2, 0]], [[10, 14, 3, 0]]), planes(d4=2, d8=2)),
    "positions around 2^63 and a hap_index beyond 2^32": (
        ([[BIG - 7, BIG + 9, FAR, 0], [BIG + 9, 2 * BIG - 1, 3, 0]], [[BIG - 9, BIG + 3, 3, 0], [BIG + 3, 2 * BIG - 2, FAR, 0]]),
        ([[BIG - 7, 2 * BIG - 1, 3, 0]], [[BIG - 8, 2 * BIG - 3, FAR, 0]]), planes(d7=10 + BIG - 12, d3=6)),
    "covered by all four only in the middle": (([[0, 60, 1, 0]], [[20, 90, 2, 0]]), ([[30, 100, 1, 0]], [[5, 40, 2, 0], [45, 70, 4, 0]]), planes(d7=10, d8=15)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_lists(gpu_lib, name):
    a, b, expect = CASES[name]
    got = check(gpu_lib, [a], [b])
    assert [g[0][0] for g in got] == expect, name


def test_one_part_against_five_hundred(gpu_lib):
    """three rows of one part against a row of 500 parts whose labels cycle through three founders; every 50th boundary keeps its label"""
    long_row, h = [], 0
    for q in range(500):
        h = h if q % 50 == 49 else (h + 1) % 3
        long_row.append([1000 + 7 * q, 1000 + 7 * (q + 1), h, 0])
    short = lambda label: [[1003, 1000 + 7 * 480 + 2, label, 0]]
    got = check(gpu_lib, [(short(1), long_row)], [(short(1), short(2))])
    sums = [g[0][0] for g in got]
    assert sum(sums) == 7 * 480 - 1 and sums[2] > 500 and sums[6] > 500 and sums[7] > 500, sums    # a1 = 1: D3; a1 = 2: D7; a1 = 0: D8


def test_rectangular_blocks(gpu_lib):
    rs = np.random.RandomState(11)
    a = T.random_rows(rs, 10); b = T.random_rows(rs, 18)
    ind_a = list(zip(a[0::2], a[1::2])); ind_b = list(zip(b[0::2], b[1::2]))
    assert np.shape(check(gpu_lib, ind_a, ind_b)) == (9, 5, 9)
    assert np.shape(check(gpu_lib, ind_a[:1], ind_b)) == (9, 1, 9)
    pa, oa = J.individuals_of(ind_a); pb, ob = J.individuals_of(ind_b)
    assert gpu_lib.dbg_identity_host(pa, oa[:1], pb, ob).shape == (9, 0, 9)
    assert gpu_lib.dbg_identity_host(pa, oa, pb, ob[:1]).shape == (9, 5, 0)


@pytest.fixture(scope="module")
def random_individuals(gpu_lib):
    """30 individuals of 1 to 40 parts per row over 12 labels: (lists, host build, truth), all pairs; computed once and left unchanged"""
    rows = T.random_rows(np.random.RandomState(20250), 60)
    pa, oa = T.lists_of(rows)
    got, want = gpu_lib.dbg_identity_host(pa, oa), J.truth(pa, oa)
    got.setflags(write=False); want.setflags(write=False)
    return rows, got, want


def test_random_individuals_all_pairs(random_individuals):
    rows, got, want = random_individuals
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert (got.reshape(9, -1).max(axis=1) > 0).all(), "the inputs were meant to reach every state"
    covered = np.array([sum(en - st for st, en, _, _ in r) for r in rows])
    assert (got.sum(axis=0) <= np.minimum.outer(np.minimum(covered[0::2], covered[1::2]), np.minimum(covered[0::2], covered[1::2]))).all()


def test_an_individual_against_itself(gpu_lib, random_individuals):
    """D1 where it is autozygous, D7 elsewhere, nothing in the other planes; the autozygous length is what the two-row walk gives"""
    rows, got, want = random_individuals
    pa, oa = T.lists_of(rows)
    shared = gpu_lib.dbg_ibd_host(pa, oa, want=(True, False, False))[0]
    both = want.sum(axis=0)
    for i in range(30):
        own = int(shared[2 * i, 2 * i + 1])
        assert got[:, i, i].tolist() == planes(d1=own, d7=int(both[i, i]) - own), i
    assert (np.diagonal(got[0]) > 0).any() and (np.diagonal(got[6]) > 0).all()


def test_transpose_identity(random_individuals):
    """D[s][i][k] == D[sigma(s)][k][i] with sigma swapping 3 <-> 5 and 4 <-> 6"""
    _, got, _ = random_individuals
    sigma = [0, 1, 4, 5, 2, 3, 6, 7, 8]
    for s in range(9):
        assert np.array_equal(got[s], got[sigma[s]].T), s
    assert np.array_equal(J.transposed(got), got)


def test_host_refusals(gpu_lib):
    """the whole messages; nothing is written"""
    pa, oa = J.individuals_of([([[1, 5, 0, 0]], [[1, 5, 0, 0]])])
    f = gpu_lib._f("dbg_identity_host")
    bp = np.full((9, 1, 1), 7, dtype=np.uint64)

    def refused(code, message, *args):
        assert f(*args) == code and gpu_lib.last_error() == message, gpu_lib.last_error()
        assert (bp == 7).all()
    refused(-1, "dbg_identity_host: null offsets", pa, None, 1, pa, oa, 1, bp)
    refused(-1, "dbg_identity_host: null offsets", pa, oa, 1, pa, None, 1, bp)
    refused(-1, "dbg_identity_host: null parts", None, oa, 1, pa, oa, 1, bp)
    refused(-1, "dbg_identity_host: the offsets of side a decrease at row 0", pa, oa[::-1].copy(), 1, pa, oa, 1, bp)
    refused(-1, "dbg_identity_host: the offsets of side b decrease at row 0", pa, oa, 1, pa, oa[::-1].copy(), 1, bp)
    refused(-1, "dbg_identity_host: bp is null", pa, oa, 1, pa, oa, 1, None)
    assert f(None, None, 0, None, None, 0, None) == 0
    assert f(pa, oa, 1, None, None, 0, None) == 0 and f(None, None, 0, pa, oa, 1, bp) == 0 and (bp == 7).all()
    assert f(pa, oa, 1, pa, oa, 1, bp) == 0 and bp.ravel().tolist() == [4, 0, 0, 0, 0, 0, 0, 0, 0]


def close(got, want):
    """one float64 division of exact integers: within 1e-15 relative of the fraction"""
    return abs(Fraction(float(got)) - want) <= abs(want) * Fraction(1, 10 ** 15)


def test_statistics_against_fractions(random_individuals):
    """identity.py on integer planes, entry by entry; a pair whose planes sum to 0 is NaN everywhere"""
    _, got, _ = random_individuals
    D = (got[:, :7, :7] * np.uint64(123_457)).copy()             # sums beyond 2^32
    D[:, 2, 3] = 0
    jac, kin, (k0, k1, k2), frat, (fa, fb) = identity.jacquard(D), identity.kinship(D), identity.ibd012(D), identity.fraternity(D), identity.inbreeding(D)
    assert jac.shape == (9, 7, 7) and jac.dtype == np.float64 and kin.shape == (7, 7)
    for i in range(7):
        for k in range(7):
            w = J.fractions_of(D, i, k)
            values = [kin[i, k], k0[i, k], k1[i, k], k2[i, k], frat[i, k], fa[i, k], fb[i, k]] + jac[:, i, k].tolist()
            if w is None:
                assert (i, k) == (2, 3) and np.isnan(values).all()
                continue
            wants = [w["kinship"], w["k0"], w["k1"], w["k2"], w["k2"], w["f_a"], w["f_b"]] + w["jacquard"]
            assert all(close(g, x) for g, x in zip(values, wants)), (i, k)
            assert w["k0"] + w["k1"] + w["k2"] == 1 and sum(w["jacquard"]) == 1
    for i in range(7):
        if i != 2:
            assert close(kin[i, i], (1 + J.fractions_of(D, i, i)["f_a"]) / 2), "an individual's kinship with itself is (1 + F) / 2"
