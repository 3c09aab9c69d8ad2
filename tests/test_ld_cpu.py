"""The LD counter of geneevolve_amd/csrc/gev_ldcount.h compiled for the host, gev_dbg_ld_host: the masking, bit-to-byte expansion, per-SNP
counts and r^2 quantum the device kernels run, with a plain integer loop in place of the matrix instruction, on haplotype-major rows
in host memory, against plain numpy.  Every comparison is exact.  No device is needed."""
import numpy as np
import pytest

from geneevolve_amd import capi, ld
from tests.ld_inputs import LDTruth, numpy_ld_counts, numpy_q40, numpy_q40_reassociated, rounding_shares, structured_rows
from tests.snp_counts_inputs import random_rows
from tests.test_snp_counts_cpu import padded

N_PEOPLE, L, L_B = 70, 200, 77
N_IND = (1, 2, 15, 16, 17, 31, 32, 33, 70)
# (a_begin, n_a, b_begin, n_b): sides of 1, 15, 16, 17, 33, 129; equal, disjoint, overlapping, rectangular
BLOCKS = [(190, 1, 0, 1), (0, 16, 0, 16), (0, 15, 100, 17), (10, 33, 30, 33), (3, 129, 60, 33), (0, 17, 5, 129), (40, 129, 40, 129), (199, 1, 0, 200)]
NAMES = ("n11", "gg", "c_a", "het_a", "hom_a", "c_b", "het_b", "hom_b")


def ind_ranges(n_ind):
    """ranges of n_ind individuals that begin at the population's first, inside a 64-haplotype word (32 individuals) and end at its last"""
    return sorted({(0, n_ind), (min(5, N_PEOPLE - n_ind), n_ind), (min(37, N_PEOPLE - n_ind), n_ind), (N_PEOPLE - n_ind, n_ind)})


@pytest.fixture(scope="module")
def population():
    """two chromosomes of the same 70 people with every allele frequency from 0 to 1; tight rows, and rows at a wider stride with
    garbage in the pad words and in the bits of the last word behind L"""
    rs = np.random.RandomState(11)
    bits = random_rows(rs, N_PEOPLE, L); bits_b = random_rows(rs, N_PEOPLE, L_B)
    wide = padded(capi.pack_rows(bits), 3, rs)
    wide[:, capi.words_for(L) - 1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(L % 64)
    wide_b = padded(capi.pack_rows(bits_b), 1, rs)
    wide_b[:, capi.words_for(L_B) - 1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(L_B % 64)
    return bits, capi.pack_rows(bits), wide, bits_b, wide_b


def check_block(lib, rows_a, bits_a, La, rows_b, bits_b, Lb, blk, i0, ni, what):
    a0, na, b0, nb = blk
    got = lib.dbg_ld_host(rows_a, La, a0, na, rows_b, Lb, b0, nb, i0, ni)
    want = numpy_ld_counts(bits_a, a0, na, bits_b, b0, nb, i0, ni)
    where = f"individuals [{i0},+{ni}), a [{a0},+{na}) b [{b0},+{nb}), {what}"
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape, name + ", " + where
        assert np.array_equal(g, w), name + ", " + where
    return got


@pytest.mark.parametrize("n_ind", N_IND)
def test_host_ld_counts_equal_numpy(gpu_lib, population, n_ind):
    bits, tight, wide, bits_b, wide_b = population
    for i0, ni in ind_ranges(n_ind):
        for blk in BLOCKS:
            check_block(gpu_lib, wide, bits, L, wide, bits, L, blk, i0, ni, "stride + 3 words of garbage")
        check_block(gpu_lib, tight, bits, L, tight, bits, L, BLOCKS[4], i0, ni, "tight rows")
        # another chromosome of the same people on side B
        for blk in ((0, 33, 0, L_B), (150, 17, 60, 17), (199, 1, 76, 1)):
            check_block(gpu_lib, wide, bits, L, wide_b, bits_b, L_B, blk, i0, ni, "two chromosomes")


def test_identities_and_monomorphic_snps(gpu_lib, population):
    bits, tight, wide, bits_b, wide_b = population
    for i0, ni in ((0, N_PEOPLE), (5, 33), (37, 1)):
        n11, gg, c, het, hom = gpu_lib.dbg_ld_host(wide, L, ind_begin=i0, n_ind=ni)[:5]
        assert np.array_equal(np.diag(n11), c) and np.array_equal(np.diag(gg), het + 4 * hom)
        assert np.array_equal(n11, n11.T) and np.array_equal(gg, gg.T)
        assert np.array_equal(c, het + 2 * hom)
        n = 2 * ni
        mono = (c == 0) | (c == n)
        assert mono.any() and (ni == 1 or (~mono).any()), "both kinds of SNP"
        # r^2 of ld.py: NaN exactly where a SNP is monomorphic, 1 on the diagonal elsewhere
        counts = ld.LDCounts(ni, *(x.astype(np.int64) for x in gpu_lib.dbg_ld_host(wide, L, ind_begin=i0, n_ind=ni)))
        r2 = ld.r2_haplotype(counts)
        assert np.array_equal(np.isnan(r2), mono[:, None] | mono[None, :])
        assert (np.diag(r2)[~mono] == 1.0).all() and np.nanmax(r2) <= 1.0
        gmono = ni * (het.astype(np.int64) + 4 * hom) == c.astype(np.int64) ** 2
        r2g = ld.r2_genotype(counts)
        assert np.array_equal(np.isnan(r2g), gmono[:, None] | gmono[None, :]) and (np.diag(r2g)[~gmono] == 1.0).all()
        dp = ld.d_prime(counts)
        assert np.array_equal(np.isnan(dp), mono[:, None] | mono[None, :]) and np.nanmax(np.abs(dp)) <= 1.0 and (np.diag(dp)[~mono] == 1.0).all()


def test_ld_py_against_the_textbook_formulas(gpu_lib, population):
    bits, tight, wide, bits_b, wide_b = population
    i0, ni, a0, na, b0, nb = 3, 60, 20, 40, 10, 50
    counts = ld.LDCounts(ni, *(x.astype(np.int64) for x in gpu_lib.dbg_ld_host(wide, L, a0, na, wide_b, L_B, b0, nb, i0, ni)))
    ha = bits[2 * i0:2 * (i0 + ni), a0:a0 + na].astype(np.float64); hb = bits_b[2 * i0:2 * (i0 + ni), b0:b0 + nb].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        want_h = np.corrcoef(ha.T, hb.T)[:na, na:] ** 2
        want_g = np.corrcoef((ha[0::2] + ha[1::2]).T, (hb[0::2] + hb[1::2]).T)[:na, na:] ** 2
    for got, want in ((ld.r2_haplotype(counts), want_h), (ld.r2_genotype(counts), want_g)):
        ok = ~np.isnan(got)
        assert ok.any() and np.array_equal(ok, ~np.isnan(want)) and np.allclose(got[ok], want[ok], rtol=1e-9, atol=1e-12)
    pa, pb = ha.mean(axis=0)[:, None], hb.mean(axis=0)[None, :]
    d = (ha.T @ hb) / (2 * ni) - pa * pb
    dmax = np.where(d >= 0, np.minimum(pa * (1 - pb), (1 - pa) * pb), np.minimum(pa * pb, (1 - pa) * (1 - pb)))
    got = ld.d_prime(counts); ok = ~np.isnan(got)
    assert np.allclose(got[ok], (d / np.where(dmax > 0, dmax, 1))[ok], rtol=1e-9, atol=1e-9)


def test_quantum_alone(gpu_lib):
    """a few thousand random triples with num^2 <= den_j den_k, and the extremes: 0, +-1, the largest counts, a zero denominator"""
    rs = np.random.RandomState(7)
    den_j = (rs.randint(1, 1 << 62, size=4000, dtype=np.int64) >> rs.randint(0, 61, size=4000)).astype(np.uint64)
    den_k = (rs.randint(1, 1 << 62, size=4000, dtype=np.int64) >> rs.randint(0, 61, size=4000)).astype(np.uint64)
    den_j[den_j == 0] = 1; den_k[den_k == 0] = 1
    lim = np.array([int(np.sqrt(float(int(a) * int(b)))) for a, b in zip(den_j, den_k)], dtype=object)
    lim = np.array([m - 1 if m * m > int(a) * int(b) else m for m, a, b in zip(lim, den_j, den_k)], dtype=object)     # floor of the root
    lim = np.array([min(int(m), (1 << 62)) for m in lim], dtype=np.int64)
    num = (lim * rs.uniform(-1, 1, size=4000)).astype(np.int64)
    num[:400] = lim[:400]; num[400:800] = -lim[400:800]
    big = 1 << 62
    ext = [(0, 1, 1), (1, 1, 1), (-1, 1, 1), (big, big, big), (-big, big, big), (1, big, big), (5, 0, 7), (5, 7, 0), (0, 0, 0), (3, 9, 1), (-3, 1, 9),
           ((1 << 31) - 1, 1 << 31, 1 << 31), (1 << 20, 1 << 62, 1), (12345678, 12345679, 12345679)]
    num = np.concatenate([num, np.array([e[0] for e in ext], dtype=np.int64)])
    den_j = np.concatenate([den_j, np.array([e[1] for e in ext], dtype=np.uint64)]); den_k = np.concatenate([den_k, np.array([e[2] for e in ext], dtype=np.uint64)])
    got = gpu_lib.dbg_ld_r2_q40_host(num, den_j, den_k)
    want = numpy_q40(num, den_j, den_k)
    assert got.dtype == np.uint64 and np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    assert got.max() == 1 << 40 and (got == 0).any() and ((got > 0) & (got < 1 << 40)).sum() > 3000
    # against the exact rational: at most half a quantum plus the three roundings of the doubles
    for i in range(0, len(num), 37):
        if den_j[i] and den_k[i]:
            exact = (int(num[i]) ** 2 << 40) / (int(den_j[i]) * int(den_k[i]))
            assert abs(int(got[i]) - exact) <= 0.5 + exact * 2.0 ** -50


def test_quantum_on_millions_of_triples_that_round(gpu_lib):
    """4 000 000 random triples with both denominators in [2^26, 2^31) and num^2 <= den_j den_k: the counts of tens of thousands of
    individuals, where num^2 and den_j den_k are no doubles.  A quantum keeps 40 bits behind the point of an r^2 of 53, so another
    order of the same operations shows in about one triple in 10^5 only: the few thousand triples above (and the 10^4 terms of a
    small score test) cannot tell r^2 = (x / dj) * (x / dk) from (x * x) / (dj * dk); these can, which is asserted of the input (the
    reassociated form differs in 122 of them)"""
    rs = np.random.RandomState(8)
    m = 4_000_000
    den_j = rs.randint(1 << 26, 1 << 31, size=m, dtype=np.int64).astype(np.uint64); den_k = rs.randint(1 << 26, 1 << 31, size=m, dtype=np.int64).astype(np.uint64)
    lim = np.floor(np.sqrt(den_j.astype(np.float64)) * np.sqrt(den_k.astype(np.float64)) * (1 - 2.0 ** -40)).astype(np.int64)
    num = (lim * rs.uniform(-1, 1, size=m)).astype(np.int64)
    want = numpy_q40(num, den_j, den_k)
    assert int(want.max()) <= 1 << 40 and int((numpy_q40_reassociated(num, den_j, den_k) != want).sum()) >= 10, "triples that tell the order of the operations"
    got = gpu_lib.dbg_ld_r2_q40_host(num, den_j, den_k)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]


@pytest.mark.parametrize("genotype", [False, True], ids=["haplotype r2", "genotype r2"])
def test_host_ld_scores_equal_numpy(gpu_lib, population, genotype):
    bits, tight, wide, bits_b, wide_b = population
    pos = np.cumsum(np.random.RandomState(3).choice([0, 1, 1, 2, 5, 40, 300], size=L)).astype(np.uint64)         # an uneven map, with ties
    for i0, ni in ((0, N_PEOPLE), (5, 33), (37, 16), (69, 1)):
        truth = LDTruth(bits, 0, L, i0, ni)
        poly = truth.poly[genotype]
        assert (~poly).any() and (poly.any() or ni == 1)            # (one individual: no genotype varies)
        for s0, ns in ((0, L), (60, 75), (199, 1)):
            windows = [ld.windows_by_count(L, s0, ns, w) for w in (0, 1, 50, L)] + [ld.windows_by_distance(pos, s0, ns, d) for d in (0, 7, 400)]
            for k, (lo, hi) in enumerate(windows):
                score, terms = gpu_lib.dbg_ld_host(wide, L, s0, ns, ind_begin=i0, n_ind=ni, win_lo=lo, win_hi=hi, genotype=genotype)
                want = truth.scores(s0, lo, hi, genotype)
                assert score.dtype == np.uint64 and terms.dtype == np.uint32
                assert np.array_equal(score, want[0]) and np.array_equal(terms, want[1]), (i0, ni, s0, ns, k)
                if k == 0:      # w = 0: exactly 2^40 per polymorphic SNP
                    assert np.array_equal(score, np.where(poly[s0:s0 + ns], np.uint64(1 << 40), np.uint64(0))) and np.array_equal(terms, poly[s0:s0 + ns])
                if k == 2 and ni > 1 and ns > 1:
                    assert truth.meaningful(s0, lo, hi, genotype)
                if k == 3:      # the whole chromosome
                    assert (lo == 0).all() and (hi == L).all() and (terms == poly.sum()).all()


def test_host_ld_scores_where_the_products_round(gpu_lib):
    """32 000 individuals x 96 SNPs in strong LD (structured_rows), individuals (3, 31965), w = 20: the input of
    test_gpu_ld.test_quanta_whose_products_round.  With the 70 people above |num| and the denominators stay below 2^13, so num^2 and
    den_j den_k are exact and only the quotient rounds; here the largest num^2 is near 2^60 and both products round in a large share of
    the terms, so that the host mirror and numpy have to agree on four roundings.  Shares of the in-window terms with a quantum strictly
    between 0 and 2^40, measured: num^2 no double 0.39 (haplotype r^2) and 0.44 (genotype r^2), den_j den_k no double 0.79 and 0.84"""
    n, Ls, i0, ni = 32000, 96, 3, 31965
    bits = structured_rows(np.random.RandomState(31), n, Ls)
    rows = capi.pack_rows(bits)
    truth = LDTruth(bits, 0, Ls, i0, ni)
    lo, hi = ld.windows_by_count(Ls, 0, Ls, 20)
    for genotype in (False, True):
        nn, dd = rounding_shares(truth, 0, lo, hi, genotype)
        print(f"genotype {genotype}: num^2 rounds in {nn:.3f} of the terms, den_j den_k in {dd:.3f}")
        assert truth.meaningful(0, lo, hi, genotype)
        assert nn >= 0.10 and dd >= 0.10, (genotype, nn, dd)
        score, terms = gpu_lib.dbg_ld_host(rows, Ls, 0, Ls, ind_begin=i0, n_ind=ni, win_lo=lo, win_hi=hi, genotype=genotype)
        want = truth.scores(0, lo, hi, genotype)
        assert np.array_equal(terms, want[1]), np.flatnonzero(terms != want[1])[:5]
        assert np.array_equal(score, want[0]), np.flatnonzero(score != want[0])[:5]


def test_windows(population):
    lo, hi = ld.windows_by_count(10, 2, 6, 3)
    assert lo.dtype == hi.dtype == np.uint32 and list(lo) == [0, 0, 1, 2, 3, 4] and list(hi) == [6, 7, 8, 9, 10, 10]
    pos = [0, 10, 10, 11, 50, 51, 51, 90]
    lo, hi = ld.windows_by_distance(pos, 1, 6, 1)
    assert list(lo) == [1, 1, 1, 4, 4, 4] and list(hi) == [4, 4, 4, 7, 7, 7]
    lo, hi = ld.windows_by_distance(np.array(pos, dtype=np.uint64), 0, 8, 40)
    assert list(lo) == [0, 0, 0, 0, 1, 3, 3, 4] and list(hi) == [4, 5, 5, 7, 8, 8, 8, 8]


def test_nothing_asked_for_and_nulls(gpu_lib, population):
    bits, tight, wide, bits_b, wide_b = population
    f = gpu_lib._f("dbg_ld_host")
    mat = np.full((4, 5), 7, dtype=np.uint32); vec = np.full(5, 7, dtype=np.uint32)
    none8 = [None] * 8

    def call(na, nb, ni, outs, tail=(None, None, 0, None, None)):
        return f(wide, wide.shape[1], L, wide, wide.shape[1], L, N_PEOPLE, 10, na, 20, nb, 3, ni, *outs, *tail)
    # no individual: zeros; no SNP on a side: nothing is touched
    assert call(4, 5, 0, [mat, None, None, None, None, vec, None, None]) == 0 and not mat.any() and not vec.any()
    mat[:] = 7; vec[:] = 7
    assert call(0, 5, 9, [mat, mat, None, None, None, vec, vec, vec]) == 0 and (mat == 7).all() and (vec == 7).all()
    assert call(4, 0, 9, [mat, mat, vec, vec, vec, None, None, None]) == 0 and (mat == 7).all() and (vec == 7).all()
    # each output on its own
    want = numpy_ld_counts(bits, 10, 4, bits, 20, 5, 3, 9)
    for k in range(8):
        out = np.full(want[k].shape, 7, dtype=np.uint32)
        outs = list(none8); outs[k] = out
        assert call(4, 5, 9, outs) == 0 and np.array_equal(out, want[k]), NAMES[k]
    # the score form: either output may be null
    lo, hi = ld.windows_by_count(L, 10, 4, 2)
    score = np.zeros(4, dtype=np.uint64); terms = np.zeros(4, dtype=np.uint32)
    truth = LDTruth(bits, 0, L, 3, 9).scores(10, lo, hi, False)
    assert call(4, 0, 9, none8, (lo, hi, 0, score, None)) == 0 and np.array_equal(score, truth[0])
    assert call(4, 0, 9, none8, (lo, hi, 0, None, terms)) == 0 and np.array_equal(terms, truth[1])


def test_host_ld_refusals(gpu_lib, population):
    bits, tight, wide, bits_b, wide_b = population

    def refused(call, word, code=-1):
        with pytest.raises(capi.GevError) as e:
            call()
        assert word in str(e.value) and e.value.code == code, str(e.value)

    refused(lambda: gpu_lib.dbg_ld_host(wide, L, L - 1, 2), "SNPs (a)")
    refused(lambda: gpu_lib.dbg_ld_host(wide, L, 0, 5, wide_b, L_B, L_B, 1), "SNPs (b)")
    refused(lambda: gpu_lib.dbg_ld_host(wide, L, 0, 5, ind_begin=N_PEOPLE - 1, n_ind=2), "individuals")
    refused(lambda: gpu_lib.dbg_ld_host(tight[:, :3], L, 0, 5), "words")
    refused(lambda: gpu_lib.dbg_ld_host(wide, L, 0, 5, tight[:, :1], L_B, 0, 5), "words")
    f = gpu_lib._f("dbg_ld_host")
    big = (1 << 30) + 1
    assert f(None, 0, 10, None, 0, 10, big, 0, 1, 0, 1, 0, big, *[None] * 8, None, None, 0, None, None) == -5
    assert "at most" in gpu_lib.last_error()
    # windows: every SNP inside its own, both arrays non-decreasing, none beyond L, none missing
    lo, hi = ld.windows_by_count(L, 50, 10, 3)
    for k, (a, b) in enumerate(((lo + 4, hi), (lo, hi - 4), (lo, hi + L), (lo[::-1].copy(), hi), (lo, np.where(np.arange(10) == 5, hi - 2, hi)))):
        refused(lambda: gpu_lib.dbg_ld_host(wide, L, 50, 10, win_lo=a, win_hi=b), "window")
    refused(lambda: gpu_lib.dbg_ld_host(wide, L, 50, 10, win_lo=lo, win_hi=None), "null window")
    refused(lambda: gpu_lib.dbg_ld_host(wide, L, 195, 5, win_lo=lo[:5], win_hi=np.full(5, L + 1, dtype=np.uint32)), "window")


# ---- ld.py on host counts ----------------------------------------------------------------------------
class HostContext:
    """the calls ld.py makes, answered from rows in host memory by the host build of the LD counter"""

    def __init__(self, lib, chroms):
        self.lib, self.chroms = lib, [capi.pack_rows(b) for b in chroms]
        self._nsnp = {(0, k): b.shape[1] for k, b in enumerate(chroms)}

    def pop_size(self, pop):
        return self.chroms[0].shape[0] // 2

    def ld_counts(self, pop, chr_a, a_begin, n_a, chr_b, b_begin, n_b, ind_begin, n_ind):
        return self.lib.dbg_ld_host(self.chroms[chr_a], self._nsnp[(0, chr_a)], a_begin, n_a, self.chroms[chr_b], self._nsnp[(0, chr_b)], b_begin, n_b, ind_begin, n_ind)

    def ld_scores(self, pop, chr, win_lo, win_hi, snp_begin, n_snps, ind_begin, n_ind, genotype):
        return self.lib.dbg_ld_host(self.chroms[chr], self._nsnp[(0, chr)], snp_begin, n_snps, ind_begin=ind_begin, n_ind=n_ind, win_lo=win_lo, win_hi=win_hi, genotype=genotype)


def test_ld_py_on_host_counts(gpu_lib, population):
    bits, tight, wide, bits_b, wide_b = population
    ctx = HostContext(gpu_lib, [bits, bits_b])
    whole = ld.counts(ctx, 0, 0)
    assert whole.n_ind == N_PEOPLE and whole.n11.shape == (L, L) and whole.n11.dtype == np.int64
    cross = ld.counts(ctx, 0, 0, (150, 20), 1, None, (7, 40))
    assert cross.gg.shape == (20, L_B) and cross.n_ind == 40
    for g, w in zip(cross[1:], numpy_ld_counts(bits, 150, 20, bits_b, 0, L_B, 7, 40)):
        assert np.array_equal(g, w)
    for genotype in (False, True):
        s = ld.ld_scores(ctx, 0, 0, w=50, snp_begin=30, n_snps=100, ind=(7, 40), genotype=genotype)
        sub = ld.counts(ctx, 0, 0, (30, 100), 0, None, (7, 40))
        r2 = ld.r2_genotype(sub) if genotype else ld.r2_haplotype(sub)
        lo, hi = ld.windows_by_count(L, 30, 100, 50)
        want = np.array([np.nansum(r2[t, lo[t]:hi[t]]) for t in range(100)])
        assert np.allclose(s.score, want, rtol=0, atol=101 * 2.0 ** -41)                   # half a quantum per term of the window
        poly = ~np.isnan(np.diag(ld.r2_genotype(whole) if genotype else ld.r2_haplotype(ld.counts(ctx, 0, 0, None, 0, None, (7, 40)))))
        if genotype:
            poly = ~np.isnan(np.diag(ld.r2_genotype(ld.counts(ctx, 0, 0, None, 0, None, (7, 40)))))
        assert np.array_equal(s.n_terms, [poly[lo[t]:hi[t]].sum() for t in range(100)])
        n = 40 if genotype else 80
        assert np.allclose(s.adjusted, s.score - (s.n_terms - s.score) / (n - 2))
        assert np.array_equal(s.score_q40, (s.score * 2.0 ** 40).astype(np.uint64))
