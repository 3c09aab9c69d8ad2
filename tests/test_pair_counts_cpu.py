"""The pairwise genotype counter of geneevolve_amd/csrc/gev_paircount.h compiled for the host, gev_dbg_pair_counts_host: the masking,
bit-to-byte expansion and finishing code the device kernels run, with a plain integer loop in place of the matrix instruction, on
haplotype-major rows in host memory, against plain numpy products.  Every comparison is exact.  No device is needed."""
import numpy as np
import pytest

from geneevolve_amd import capi, relatedness
from tests.pair_counts_inputs import numpy_ind_counts, numpy_pair_counts
from tests.snp_counts_inputs import random_rows
from tests.test_snp_counts_cpu import padded, snp_ranges

N_IND = (1, 2, 15, 16, 17, 33, 70)
LOCI = (1, 31, 64, 65, 127, 129, 5000)


def ind_ranges(n):
    """(a_begin, n_a, b_begin, n_b): equal, disjoint, overlapping, one individual, different lengths"""
    r = {(0, n, 0, n), (0, 1, n - 1, 1), (n - 1, 1, 0, n), (0, n, n // 2, 1)}
    if n >= 4:
        h = n // 2
        r |= {(0, h, h, n - h), (h, n - h, 0, h), (0, h + 1, h - 1, n - h + 1), (1, n - 2, 0, n), (n // 3, 2, 0, n - 1)}
    return sorted(r)


def check(lib, rows, bits, L, s0, ns, ab, what):
    a0, na, b0, nb = ab
    het, hom, hethet, opphom, dot = lib.dbg_pair_counts_host(rows, L, s0, ns, a0, na, b0, nb)
    want_ind = numpy_ind_counts(bits, s0, ns)
    want = numpy_pair_counts(bits, s0, ns, a0, na, b0, nb)
    where = f"{bits.shape[0] // 2} individuals x {L} SNPs, SNPs [{s0},{s0 + ns}), a [{a0},+{na}) b [{b0},+{nb}), {what}"
    assert het.dtype == hom.dtype == hethet.dtype == opphom.dtype == dot.dtype == np.uint32
    assert hethet.shape == opphom.shape == dot.shape == (na, nb)
    assert np.array_equal(het, want_ind[0]), "n_het, " + where
    assert np.array_equal(hom, want_ind[1]), "n_hom_alt, " + where
    assert np.array_equal(hethet, want[0]), "n_hethet, " + where
    assert np.array_equal(opphom, want[1]), "n_opphom, " + where
    assert np.array_equal(dot, want[2]), "dot, " + where


@pytest.mark.parametrize("L", LOCI)
@pytest.mark.parametrize("n_ind", N_IND)
def test_host_pair_counts_equal_numpy(gpu_lib, n_ind, L):
    rs = np.random.RandomState(1000 * L + n_ind)
    bits = random_rows(rs, n_ind, L)
    words = capi.pack_rows(bits)
    wide = padded(words, 3, rs)
    whole = (0, n_ind, 0, n_ind)
    for s0, ns in snp_ranges(L):
        for rows, what in ((words, "tight rows"), (wide, "stride + 3 words of garbage")):
            check(gpu_lib, rows, bits, L, s0, ns, whole, what)
    # every shape of the two ranges of individuals, over the whole SNP range and over one that begins and ends inside a word
    for s0, ns in {(0, L), (min(5, L - 1), max(1, min(L - 6, 119)))}:
        if s0 + ns <= L:
            for ab in ind_ranges(n_ind):
                check(gpu_lib, wide, bits, L, s0, ns, ab, "stride + 3 words of garbage")


def test_garbage_beyond_L_in_the_last_word_is_not_counted(gpu_lib):
    rs = np.random.RandomState(5)
    n_ind, L = 33, 70
    bits = random_rows(rs, n_ind, L)
    words = capi.pack_rows(bits).copy()
    words[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(L - 64)
    for s0, ns in ((0, L), (64, 6), (69, 1), (3, 66)):
        check(gpu_lib, words, bits, L, s0, ns, (0, n_ind, 0, n_ind), "pad bits set")
        check(gpu_lib, words, bits, L, s0, ns, (3, 17, 10, 23), "pad bits set")


def test_extreme_rows(gpu_lib):
    """everybody 1/1 (dot = 4 L, the largest), everybody 0/1, and the two halves opposite homozygotes (n_opphom = L)"""
    L, n = 129, 4
    one = np.ones((2 * n, L), dtype=np.uint8)
    het = one.copy(); het[1::2] = 0
    opp = one.copy(); opp[2 * (n // 2):] = 0
    for bits in (one, het, opp):
        check(gpu_lib, capi.pack_rows(bits), bits, L, 0, L, (0, n, 0, n), "extreme rows")
    assert gpu_lib.dbg_pair_counts_host(capi.pack_rows(one), L)[4][0, 0] == 4 * L
    assert gpu_lib.dbg_pair_counts_host(capi.pack_rows(opp), L)[3][0, n - 1] == L


def test_nothing_asked_for(gpu_lib):
    f = gpu_lib._f("dbg_pair_counts_host")
    words = capi.pack_rows(np.ones((4, 100), dtype=np.uint8))
    vec = np.full(2, 7, dtype=np.uint32); mat = np.full((2, 2), 7, dtype=np.uint32)
    # no SNP: zeros everywhere
    assert f(words, 2, 2, 100, 40, 0, 0, 2, 0, 2, vec, vec, mat, mat, mat) == 0
    assert not vec.any() and not mat.any()
    # no pair: the matrices are not touched (null is fine), the vectors are written
    mat[:] = 7
    assert f(words, 2, 2, 100, 0, 100, 1, 0, 0, 2, vec, None, None, None, None) == 0
    assert list(vec) == [0, 0] and (mat == 7).all()
    # each output may be null
    assert f(words, 2, 2, 100, 0, 100, 0, 2, 0, 2, None, None, None, None, mat) == 0
    assert (mat == 400).all()


def test_host_pair_counts_refusals(gpu_lib):
    f = gpu_lib._f("dbg_pair_counts_host")
    words = np.zeros((4, 2), dtype=np.uint64)
    vec = np.zeros(2, dtype=np.uint32); mat = np.zeros((2, 2), dtype=np.uint32)

    def rc(bits, stride, n_ind, L, s0, ns, a0, na, b0, nb):
        return f(bits, stride, n_ind, L, s0, ns, a0, na, b0, nb, vec, vec, mat, mat, mat)
    assert rc(words, 2, 2, 100, 90, 11, 0, 2, 0, 2) == -1 and "SNPs" in gpu_lib.last_error() and "beyond" in gpu_lib.last_error()
    assert rc(words, 2, 2, 100, 0, 100, 1, 2, 0, 2) == -1 and "(a)" in gpu_lib.last_error()
    assert rc(words, 2, 2, 100, 0, 100, 0, 2, 2, 1) == -1 and "(b)" in gpu_lib.last_error()
    assert rc(words, 1, 2, 100, 0, 100, 0, 2, 0, 2) == -1 and "words" in gpu_lib.last_error()
    assert rc(None, 0, 2, (1 << 30) + 1, 0, (1 << 30) + 1, 0, 2, 0, 2) == -5 and "at most" in gpu_lib.last_error()


# ---- relatedness.py on host counts ----------------------------------------------------------------
class HostContext:
    """the calls relatedness.py makes, answered from rows in host memory: the host build of the pair counter, numpy for the rest"""

    def __init__(self, lib, chroms):
        self.lib, self.chroms = lib, chroms                                  # chroms: one uint8 [2 N][L] per chromosome
        self.nchr = len(chroms)
        self._nsnp = {(0, k): b.shape[1] for k, b in enumerate(chroms)}

    def pop_size(self, pop):
        return self.chroms[0].shape[0] // 2

    def active_chrs(self):
        return list(range(self.nchr))

    def snp_genotype_counts(self, pop, chr):
        return self.lib.dbg_snp_counts_host(capi.pack_rows(self.chroms[chr]), self.chroms[chr].shape[1])

    def ind_genotype_counts(self, pop, chr, ind_begin=0, n_ind=None, weight=None):
        b = self.chroms[chr]
        het, hom = self.lib.dbg_pair_counts_host(capi.pack_rows(b), b.shape[1], n_a=0, n_b=0)[:2]
        sl = slice(ind_begin, ind_begin + n_ind)
        if weight is None:
            return het[sl], hom[sl]
        g = (b[0::2].astype(object) + b[1::2].astype(object))[sl]
        return het[sl], hom[sl], np.array([int(v) for v in g @ weight.astype(object)], dtype=np.uint64)

    def pair_genotype_counts(self, pop, chr, a_begin=0, n_a=None, b_begin=0, n_b=None):
        b = self.chroms[chr]
        return self.lib.dbg_pair_counts_host(capi.pack_rows(b), b.shape[1], 0, None, a_begin, n_a, b_begin, n_b)[2:]


@pytest.fixture(scope="module")
def host_ctx(gpu_lib):
    rs = np.random.RandomState(77)
    return HostContext(gpu_lib, [random_rows(rs, 37, L) for L in (301, 64, 1000)])


def test_relatedness_pair_counts_sum_over_chromosomes(host_ctx):
    pc = relatedness.pair_counts(host_ctx, 0, (3, 20), (11, 26))
    want = [sum(m) for m in zip(*(numpy_pair_counts(b, 0, None, 3, 20, 11, 26) for b in host_ctx.chroms))]
    ind = [sum(v.astype(np.int64) for v in vs) for vs in zip(*(numpy_ind_counts(b) for b in host_ctx.chroms))]
    assert pc.n_snps == 1365
    for got, w in zip((pc.n_hethet, pc.n_opphom, pc.dot), want):
        assert got.dtype == np.int64 and np.array_equal(got, w)
    assert np.array_equal(pc.het_a, ind[0][3:23]) and np.array_equal(pc.hom_b, ind[1][11:37])
    # IBS distance is sum |g_i - g_k|
    g = np.concatenate([(b[0::2].astype(np.int64) + b[1::2]) for b in host_ctx.chroms], axis=1)
    sum_abs = np.abs(g[3:23, None, :] - g[None, 11:37, :]).sum(axis=2)
    assert np.array_equal(relatedness.ibs_distance(pc), sum_abs)


def test_king_self_kinship_is_one_half(host_ctx):
    pc = relatedness.pair_counts(host_ctx, 0)
    for robust in (False, True):
        k = relatedness.king_kinship(pc, robust=robust)
        assert k.shape == (37, 37) and np.array_equal(np.diag(k), np.full(37, 0.5))
    # the formulas, entry by entry in Python integers and float64
    i, j = 4, 30
    num = int(pc.n_hethet[i, j]) - 2 * int(pc.n_opphom[i, j]); hi, hj = int(pc.het_a[i]), int(pc.het_b[j]); m = min(hi, hj)
    assert relatedness.king_kinship(pc)[i, j] == num / (hi + hj)
    assert relatedness.king_kinship(pc, robust=True)[i, j] == num / (2.0 * m) + 0.5 - (hi + hj) / (4.0 * m)


def test_king_is_nan_without_heterozygous_loci(gpu_lib):
    ctx = HostContext(gpu_lib, [np.ones((6, 50), dtype=np.uint8)])
    pc = relatedness.pair_counts(ctx, 0)
    assert np.isnan(relatedness.king_kinship(pc)).all() and np.isnan(relatedness.king_kinship(pc, robust=True)).all()


def test_grm_vanraden_against_python_integers(host_ctx):
    from fractions import Fraction
    a, b = (0, 37), (5, 20)
    grm = relatedness.grm_vanraden(host_ctx, 0, a, b)
    N = 37
    g = np.concatenate([(c[0::2].astype(object) + c[1::2].astype(object)) for c in host_ctx.chroms], axis=1)
    c = g.sum(axis=0)
    sum_c2 = int((c * c).sum()); den = Fraction(int((c * (2 * N - c)).sum()), 2 * N * N)
    s = g @ c
    dot = g[a[0]:a[0] + a[1]] @ g[b[0]:b[0] + b[1]].T
    eps = np.finfo(np.float64).eps
    assert grm.shape == (37, 20)
    for i in range(a[1]):
        for k in range(b[1]):
            si, sk = int(s[a[0] + i]), int(s[b[0] + k])
            exact = (Fraction(int(dot[i, k])) - Fraction(si + sk, N) + Fraction(sum_c2, N * N)) / den
            bound = 8 * eps * (abs(int(dot[i, k])) + abs(si + sk) / N + sum_c2 / (N * N)) / float(den)
            assert abs(grm[i, k] - float(exact)) <= bound, (i, k, grm[i, k], float(exact), bound)
    # Z Z' straight from the centred genotypes, in floating point: the identity itself
    p = c.astype(np.float64) / (2 * N)
    zc = g.astype(np.float64) - 2 * p
    assert np.allclose(grm, (zc[a[0]:a[0] + a[1]] @ zc[b[0]:b[0] + b[1]].T) / (2 * p * (1 - p)).sum(), rtol=1e-9, atol=1e-9)


def test_wsum_needs_its_64_bits(gpu_lib):
    """weights up to 2^32 - 1 on the host arithmetic of the header (gev_pc_weighted through the stand-alone check has the same cases):
    here the Python side -- relatedness keeps such sums as integers"""
    ctx = HostContext(gpu_lib, [np.ones((4, 70), dtype=np.uint8)])
    w = np.full(70, 0xFFFFFFFF, dtype=np.uint32)
    ws = ctx.ind_genotype_counts(0, 0, 0, 2, weight=w)[2]
    assert ws.dtype == np.uint64 and int(ws[0]) == 2 * 70 * 0xFFFFFFFF > 1 << 32
