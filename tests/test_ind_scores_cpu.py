"""The score arithmetic of geneevolve_amd/csrc/gev_indscore.h compiled for the host, gev_dbg_ind_scores_host: the masking, the digit
split, the byte order of both operands and the recombination the device kernels run, with a plain integer loop in place of the matrix
instruction, on haplotype-major rows in host memory, against plain numpy (tests/ind_scores_inputs.py) -- by equality.  Then
scores.quantise_weights in exact rationals.  No device is needed."""
from fractions import Fraction

import numpy as np
import pytest

from geneevolve_amd import capi, scores
from tests.ind_scores_inputs import (EDGE_WEIGHTS, L, N_PEOPLE, NAMES, STEP, W_MAX, genotypes, numpy_scores, one_hot_value, one_hot_weights,
                                     population_rows, random_weights)
from tests.test_snp_counts_cpu import padded

N_IND = (1, 15, 16, 17, 127, 128, 129, 150)
# (snp_begin, n_snps): 1, 15, 16, 17, 63, 64, 65, 255, 256, 257 SNPs; beginning inside a word and on one; across the edges of a word
# (64 SNPs), of a step (256) and of a slice (4096)
SNP_RANGES = [(L - 1, 1), (4095, 1), (56, 15), (4090, 16), (0, 17), (1, 63), (64, 64), (63, 65), (4033, 64), (130, 255), (4096, 256), (3, 256), (250, 257), (4000, 257),
              (8100, L - 8100)]
N_SCORES = (0, 1, 3, 4, 5, 17)


def ind_ranges(n_ind):
    """ranges of n_ind individuals that begin at the population's first, inside it, and that end at its last"""
    return sorted({(min(b, N_PEOPLE - n_ind), n_ind) for b in (0, 9, N_PEOPLE)})


@pytest.fixture(scope="module")
def population():
    """150 people x 8269 SNPs: the 0/1/2 matrix, the packed rows, and the packed rows at a wider stride with garbage in the pad words
    and in the bits of the last word behind L"""
    bits = population_rows()
    wide = padded(capi.pack_rows(bits), 2, np.random.RandomState(4))
    wide[:, capi.words_for(L) - 1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(L % 64)
    return genotypes(bits), capi.pack_rows(bits), wide


def check(lib, rows, geno, w, s0, ns, i0, ni, what="", row_L=L):
    got = lib.dbg_ind_scores_host(rows, row_L, w, s0, ns, i0, ni)
    want = numpy_scores(geno, s0, ns, i0, ni, w)
    where = f"individuals [{i0},+{ni}), SNPs [{s0},+{ns}), {np.atleast_2d(w).shape[0]} columns {what}"
    for name, g, x in zip(NAMES, got, want):
        assert g.dtype == np.int64 and g.shape == x.shape, name + ", " + where
        assert np.array_equal(g, x), f"{name}, {where}: differs at {np.argwhere(g != x)[:5].tolist()}"
    return got


@pytest.mark.parametrize("n_ind", N_IND)
def test_host_scores_equal_numpy(gpu_lib, population, n_ind):
    geno, tight, wide = population
    rs = np.random.RandomState(100 + n_ind)
    k = 0
    for i0, ni in ind_ranges(n_ind):
        for s0, ns in SNP_RANGES:
            check(gpu_lib, wide, geno, random_weights(rs, N_SCORES[k % len(N_SCORES)], ns), s0, ns, i0, ni, "stride + 2 words of garbage"); k += 1
        check(gpu_lib, tight, geno, random_weights(rs, 5, 257), 3, 257, i0, ni, "tight rows")
    i0, ni = ind_ranges(n_ind)[-1]
    check(gpu_lib, wide, geno, random_weights(rs, 4 if n_ind % 2 else 5, L), 0, L, i0, ni, "the whole row")


@pytest.mark.parametrize("n_scores", N_SCORES)
def test_every_number_of_columns_on_every_snp_range(gpu_lib, population, n_scores):
    geno, tight, wide = population
    rs = np.random.RandomState(7 + n_scores)
    for s0, ns in SNP_RANGES + [(0, L)]:
        check(gpu_lib, wide, geno, random_weights(rs, n_scores, ns), s0, ns, 3, 40)
    if n_scores == 1:
        check(gpu_lib, wide, geno, random_weights(rs, 1, 300)[0], 5, 300, 3, 40, "one column as a vector")


@pytest.mark.parametrize("first", [0, 3, 64, 100, 4096, L - STEP], ids=lambda b: f"first SNP {b}")
def test_one_hot_columns_tell_the_byte_order(gpu_lib, population, first):
    """for every byte position p of a step (4 words x 4 matrix steps x 16 bytes) a column whose only weight sits at SNP first + p, a
    different value with four non-zero digits at each: gscore[p][i] = g_ip w_p, so one misplaced byte of the weight operand is one wrong
    entry.  The 256 positions from the first SNP of a word, of a step and of a slice, from inside a word, and at the row's end; in a
    range that begins with them and in one that begins before them, inside a word"""
    geno, tight, wide = population
    vals = np.array([one_hot_value(p) for p in range(STEP)], dtype=np.int64)
    for s0 in sorted({first, max(first - 37, 0)}):
        ns = min(first + STEP + 70, L) - s0
        gscore, hetscore = check(gpu_lib, wide, geno, one_hot_weights(ns, first - s0), s0, ns, 0, N_PEOPLE, f"one-hot from {first}")
        g = geno[:, first:first + STEP].T
        assert np.array_equal(gscore, g * vals[:, None]) and np.array_equal(hetscore, (g == 1) * vals[:, None])
        assert (g == 1).any(axis=0).all() and (g == 2).any(axis=0).all(), "every individual tells the positions apart"
    if first == 100:
        check(gpu_lib, wide, geno, one_hot_weights(L, first), 0, L, 20, 17, "one-hot in the whole row")


def test_digit_carry_edges(gpu_lib, population):
    """weights at +-2^30, 0, +-1, +-127, +-128, +-129, +-32768: alone in a column (one value at every SNP), and every edge at every
    position of a word"""
    geno, tight, wide = population
    for s0, ns in ((0, 300), (4000, 200), (60, 5)):
        alone = np.repeat(np.array(EDGE_WEIGHTS, dtype=np.int32)[:, None], ns, axis=1)
        gscore = check(gpu_lib, wide, geno, alone, s0, ns, 10, 70, "one edge value each")[0]
        c = geno[10:80, s0:s0 + ns].sum(axis=1)
        assert np.array_equal(gscore, np.array(EDGE_WEIGHTS, dtype=np.int64)[:, None] * c[None, :])
        rolled = np.stack([np.roll(np.resize(np.array(EDGE_WEIGHTS, dtype=np.int32), ns), k) for k in range(len(EDGE_WEIGHTS))])
        check(gpu_lib, wide, geno, rolled, s0, ns, 10, 70, "the edges rolled over the SNPs")


def test_rows_of_one_genotype(gpu_lib):
    """everybody 0/0, everybody 1/1, everybody heterozygous (either haplotype carrying the allele): the scores are 0, twice the column's
    sum, and the column's sum in both outputs"""
    rs = np.random.RandomState(9)
    n, Ls = 20, 700
    w = random_weights(rs, 5, 600)
    total = w.astype(np.int64).sum(axis=1)[:, None] * np.ones((1, n), dtype=np.int64)
    pick = rs.randint(0, 2, size=(n, Ls)).astype(np.uint8)
    for name, a, b, want in (("0/0", 0 * pick, 0 * pick, (0 * total, 0 * total)), ("1/1", 0 * pick + 1, 0 * pick + 1, (2 * total, 0 * total)),
                             ("0/1", pick, 1 - pick, (total, total))):
        bits = np.empty((2 * n, Ls), dtype=np.uint8)
        bits[0::2], bits[1::2] = a, b
        got = check(gpu_lib, capi.pack_rows(bits), genotypes(bits), w, 50, 600, 0, n, name, row_L=Ls)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name


def test_nothing_asked_for_and_nulls(gpu_lib, population):
    geno, tight, wide = population
    f = gpu_lib._f("dbg_ind_scores_host")
    w = random_weights(np.random.RandomState(3), 3, 70)
    want = numpy_scores(geno, 10, 70, 20, 9, w)

    def call(ns, ni, nsc, outs, weight=w):
        return f(wide, wide.shape[1], N_PEOPLE, L, 10, ns, 20, ni, weight, nsc, *outs)
    both = [np.full((3, 9), 7, dtype=np.int64) for _ in range(2)]
    assert call(70, 0, 3, both) == 0 and all((a == 7).all() for a in both), "no individual: nothing is touched"
    assert call(0, 9, 3, both, None) == 0 and not any(a.any() for a in both), "no SNP: zeros"
    both = [np.full((3, 9), 7, dtype=np.int64) for _ in range(2)]
    assert call(70, 9, 0, both, None) == 0 and all((a == 7).all() for a in both), "no column: matrices of no rows, nothing to write"
    for k in range(2):                                       # each output on its own
        out = np.full((3, 9), 7, dtype=np.int64)
        outs = [None, None]; outs[k] = out
        assert call(70, 9, 3, outs) == 0 and np.array_equal(out, want[k]), NAMES[k]
        only = gpu_lib.dbg_ind_scores_host(wide, L, w, 10, 70, 20, 9, want=(k == 0, k == 1))
        assert only[1 - k] is None and np.array_equal(only[k], want[k])
    assert call(70, 9, 3, [None, None]) == 0
    got = gpu_lib.dbg_ind_scores_host(wide, L, np.zeros((0, 70), dtype=np.int32), 10, 70, 20, 9)
    assert got[0].shape == got[1].shape == (0, 9)


def test_host_scores_refusals(gpu_lib, population):
    geno, tight, wide = population
    w = np.zeros((2, 5), dtype=np.int32)

    def refused(call, word, code=-1):
        with pytest.raises(capi.GevError) as e:
            call()
        assert word in str(e.value) and e.value.code == code, str(e.value)

    refused(lambda: gpu_lib.dbg_ind_scores_host(wide, L, np.zeros((2, 2), dtype=np.int32), L - 1, 2, 0, 5), "SNPs")
    refused(lambda: gpu_lib.dbg_ind_scores_host(wide, L, w, 0, 5, N_PEOPLE - 4, 5), "individuals")
    refused(lambda: gpu_lib.dbg_ind_scores_host(tight[:, :3], L, w, 0, 5, 0, 5), "words")
    for bad in (W_MAX + 1, -W_MAX - 1, -(1 << 31)):
        w1 = w.copy(); w1[1, 3] = bad
        refused(lambda: gpu_lib.dbg_ind_scores_host(wide, L, w1, 0, 5, 0, 5), "weight")
    w1 = w.copy(); w1[0, 0] = W_MAX; w1[1, 4] = -W_MAX
    gpu_lib.dbg_ind_scores_host(wide, L, w1, 0, 5, 0, 5)
    f = gpu_lib._f("dbg_ind_scores_host")
    out = np.zeros((2, 5), dtype=np.int64)
    assert f(wide, wide.shape[1], N_PEOPLE, L, 0, 5, 0, 5, None, 2, out, None) == -1
    assert "null weight" in gpu_lib.last_error()
    big = (1 << 22) + 1
    assert f(None, 0, 10, big, 0, big, 0, 1, None, 1, None, None) == -5
    assert "at most" in gpu_lib.last_error()
    assert f(wide, wide.shape[1], N_PEOPLE, L, 0, 0, 0, 5, None, 2, out, None) == 0, "no SNP: the weights are not read"


# ---- scores.py ---------------------------------------------------------------------------------------
def test_quantise_weights_round_trips():
    """|q scale - beta| <= scale / 2, decided in exact rationals; the largest |beta| maps to +-2^bits; nothing is centred"""
    rs = np.random.RandomState(5)
    beta = np.stack([rs.normal(0.0, 0.01, 500), 3.0 + rs.standard_cauchy(500) * 1e-3, rs.uniform(-1, 1, 500) * 1e12, np.zeros(500)])
    for bits in (30, 12):
        q, scale = scores.quantise_weights(beta, bits)
        assert q.dtype == np.int32 and q.shape == beta.shape and np.abs(q.astype(np.int64)).max(axis=1).tolist() == [1 << bits] * 3 + [0] and scale[3] == 1.0
        assert q[1].min() > 0, "a column of positive weights stays positive: no centring"
        for t in range(3):
            half = Fraction(float(scale[t])) / 2
            for j in range(500):
                assert abs(int(q[t, j]) * Fraction(float(scale[t])) - Fraction(float(beta[t, j]))) <= half, (bits, t, j)
    q, scale = scores.quantise_weights(beta[0])
    assert q.shape == (1, 500) and scale.shape == (1,)


class HostContext:
    """the calls scores.py makes, answered from rows in host memory by the host build of the scores; chromosome c holds the SNPs
    [at[c], at[c + 1]) of the rows"""

    def __init__(self, lib, rows, at):
        self.lib, self.rows, self.at = lib, rows, at
        self._nsnp = {(0, c): at[c + 1] - at[c] for c in range(len(at) - 1)}

    def pop_size(self, pop):
        return self.rows.shape[0] // 2

    def ind_scores(self, pop, chr, weight, snp_begin, n_snps, ind_begin, n_ind, want=(True, True)):
        return self.lib.dbg_ind_scores_host(self.rows, self.at[-1], weight, self.at[chr] + snp_begin, n_snps, ind_begin, n_ind, want=want)


def test_scores_over_chromosomes_and_split_ranges(gpu_lib, population, monkeypatch):
    """scores.sums adds the chromosomes, and splits a chromosome longer than one call takes (the limit lowered to 1000 SNPs here);
    scores.prs is the float score within the quantisation: |q scale - beta| <= scale / 2 at each of at most 2 n_snps allele copies"""
    geno, tight, wide = population
    at = [0, 3000, 3001, L]
    ctx = HostContext(gpu_lib, wide, at)
    rs = np.random.RandomState(8)
    q = {c: random_weights(rs, 3, at[c + 1] - at[c]) for c in range(3)}
    whole = np.concatenate([q[c] for c in range(3)], axis=1)
    want = numpy_scores(geno, 0, L, 5, 100, whole)
    got = scores.sums(ctx, 0, q, (5, 100))
    assert all(np.array_equal(g, x) for g, x in zip(got, want))
    monkeypatch.setattr(scores, "MAX_SNPS", 1000)
    got = scores.sums(ctx, 0, q, (5, 100))
    assert all(np.array_equal(g, x) for g, x in zip(got, want)), "ranges of 1000 SNPs added"
    only = scores.sums(ctx, 0, {1: q[1]}, want=(False, True))
    assert only[0] is None and np.array_equal(only[1], numpy_scores(geno, 3000, 1, 0, N_PEOPLE, q[1])[1])
    beta = {c: rs.normal(0, 1, (2, at[c + 1] - at[c])) for c in range(3)}
    delta = {c: rs.normal(0, 0.3, (2, at[c + 1] - at[c])) for c in range(3)}
    b = np.concatenate([beta[c] for c in range(3)], axis=1); d = np.concatenate([delta[c] for c in range(3)], axis=1)
    g = geno.astype(np.float64)
    add = scores.prs(ctx, 0, beta)
    bound = 2 * L * np.abs(b).max(axis=1) / float(1 << 31) + 1e-12 * np.abs(b @ g.T).max()
    assert add.shape == (2, N_PEOPLE) and (np.abs(add - b @ g.T) <= bound[:, None]).all()
    both = scores.prs(ctx, 0, beta, dominance_by_chr=delta)
    bound_d = L * np.abs(d).max(axis=1) / float(1 << 31)
    assert (np.abs(both - b @ g.T - d @ (g == 1).T) <= (bound + bound_d)[:, None]).all()
