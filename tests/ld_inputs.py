"""Shared by the LD tests (test_ld_cpu.py, test_gpu_ld.py): the plain numpy statement of the SNP-pair counts, of the r^2 quantum and of
an LD score.  The matrix products go through float64 (exact below 2^53); the quantum does the same IEEE double operations as
gev_ld_r2_q40, one at a time."""
import numpy as np

Q40 = float(1 << 40)


def numpy_snp_side(bits01, s0, ns, i0, ni):
    """unpacked haplotype rows -> (haplotypes float64 [2 ni][ns], genotypes float64 [ni][ns], c, n_het, n_hom_alt int64 [ns]) of SNPs
    [s0, +ns) over individuals [i0, +ni)"""
    h = bits01[2 * i0:2 * (i0 + ni), s0:s0 + ns].astype(np.float64)
    g = h[0::2] + h[1::2]
    return h, g, h.sum(axis=0).astype(np.int64), (g == 1).sum(axis=0).astype(np.int64), (g == 2).sum(axis=0).astype(np.int64)


def numpy_ld_counts(bits_a, a0, na, bits_b, b0, nb, i0, ni):
    """-> (n11, gg, c_a, het_a, hom_a, c_b, het_b, hom_b), int64"""
    ha, ga, ca, hea, hoa = numpy_snp_side(bits_a, a0, na, i0, ni)
    hb, gb, cb, heb, hob = numpy_snp_side(bits_b, b0, nb, i0, ni)
    return (ha.T @ hb).astype(np.int64), (ga.T @ gb).astype(np.int64), ca, hea, hoa, cb, heb, hob


def numpy_q40(num, den_j, den_k):
    """the r^2 quantum of int64 num and den_j, den_k >= 0 (broadcast): rint(((double)num * (double)num) / ((double)den_j * (double)den_k)
    * 2^40) as uint64, 0 where a denominator is 0"""
    num, den_j, den_k = np.broadcast_arrays(np.asarray(num, dtype=np.int64), np.asarray(den_j, dtype=np.uint64), np.asarray(den_k, dtype=np.uint64))
    x = num.astype(np.float64)
    nn = x * x
    dd = den_j.astype(np.float64) * den_k.astype(np.float64)
    ok = (den_j != 0) & (den_k != 0)
    r2 = np.divide(nn, dd, out=np.zeros_like(nn), where=ok)
    return np.where(ok, np.rint(r2 * Q40), 0.0).astype(np.uint64)


def numpy_q40_reassociated(num, den_j, den_k):
    """what the quantum is NOT: (x / den_j) * (x / den_k), the same r^2 in another order of the double operations.  It differs from
    numpy_q40 in about one term in 10^5 once num^2 and den_j den_k round, and in none while they are exact and small; the tests that
    mean to tell the two apart assert that their input does"""
    num, den_j, den_k = np.broadcast_arrays(np.asarray(num, dtype=np.int64), np.asarray(den_j, dtype=np.uint64), np.asarray(den_k, dtype=np.uint64))
    ok = (den_j != 0) & (den_k != 0)
    x, dj, dk = num.astype(np.float64), np.where(ok, den_j, 1).astype(np.float64), np.where(ok, den_k, 1).astype(np.float64)
    return np.where(ok, np.rint((x / dj) * (x / dk) * Q40), 0.0).astype(np.uint64)


def numpy_num_den(counts, ni, genotype):
    """(num [na][nb], den_a [na], den_b [nb]) of numpy_ld_counts' result, int64"""
    n11, gg, ca, hea, hoa, cb, heb, hob = counts
    if genotype:
        return ni * gg - ca[:, None] * cb[None, :], ni * (hea + 4 * hoa) - ca * ca, ni * (heb + 4 * hob) - cb * cb
    n = 2 * ni
    return n * n11 - ca[:, None] * cb[None, :], ca * (n - ca), cb * (n - cb)


def structured_rows(rs, n_ind, L):
    """uint8 [2 * n_ind][L] of 0/1 in strong LD: 12 ancestral haplotypes of fair coin bits; an individual's first haplotype copies a
    random ancestor, its second the same one with probability 0.7 and another random one otherwise; every bit is then flipped with
    probability 0.02.  Column 0 is all 0 and column L // 2 all 1.  With tens of thousands of individuals the numerators and
    denominators of r^2 are far beyond 2^26.5, so their products are no doubles and every operation of the quantum rounds"""
    anc = rs.randint(0, 2, size=(12, L)).astype(np.uint8)
    first = rs.randint(0, 12, size=n_ind)
    second = np.where(rs.random_sample(n_ind) < 0.7, first, rs.randint(0, 12, size=n_ind))
    rows = np.empty((2 * n_ind, L), dtype=np.uint8)
    rows[0::2] = anc[first]; rows[1::2] = anc[second]
    rows ^= (rs.random_sample((2 * n_ind, L)) < 0.02).astype(np.uint8)
    rows[:, 0] = 0; rows[:, L // 2] = 1
    return rows


def rounding_shares(truth, snp_begin, win_lo, win_hi, genotype):
    """of the in-window terms of SNPs snp_begin + t whose quantum lies strictly between 0 and 2^40: (the share whose num^2 is not a
    double, the share whose den_j den_k is not a double), decided in Python integers.  (double)num and (double)den are exact here."""
    num, den_a, den_b = numpy_num_den(truth.counts, truth.ni, genotype)
    q = truth.q[genotype]
    terms = nn = dd = 0
    for t, (lo, hi) in enumerate(zip(win_lo, win_hi)):
        j = snp_begin + t - truth.s0
        for k in range(int(lo) - truth.s0, int(hi) - truth.s0):
            if not 0 < int(q[j, k]) < 1 << 40:
                continue
            x, dj, dk = int(num[j, k]), int(den_a[j]), int(den_b[k])
            assert abs(x) < 1 << 53 and dj < 1 << 53 and dk < 1 << 53
            terms += 1
            nn += int(float(x) * float(x)) != x * x
            dd += int(float(dj) * float(dk)) != dj * dk
    assert terms, "a quantum strictly between 0 and 2^40"
    return nn / terms, dd / terms


class _Lazy:
    """truth.q[genotype] / truth.poly[genotype]"""

    def __init__(self, truth, which):
        self.truth, self.which = truth, which

    def __getitem__(self, genotype):
        return self.truth.kind(bool(genotype))[self.which]


class LDTruth:
    """SNPs [s0, +ns) of one chromosome against themselves over individuals [i0, +ni): the counts and the quanta of both kinds of r^2,
    computed once and sliced by the tests (indices are SNP indices of the chromosome)"""

    def __init__(self, bits01, s0, ns, i0, ni):
        self.s0, self.ns, self.ni, self._kinds = s0, ns, ni, {}
        self.counts = numpy_ld_counts(bits01, s0, ns, bits01, s0, ns, i0, ni)
        self.q, self.poly = _Lazy(self, 0), _Lazy(self, 1)

    def kind(self, genotype):
        """(quanta uint64 [ns][ns], polymorphic bool [ns]) of one kind of r^2, computed when first asked for"""
        if genotype not in self._kinds:
            self._kinds[genotype] = (self.quanta(genotype), numpy_num_den(self.counts, self.ni, genotype)[1] > 0)
        return self._kinds[genotype]

    def quanta(self, genotype, quantum=numpy_q40):
        """uint64 [ns][ns]: quantum(num, den_j, den_k) of every pair"""
        num, den_a, den_b = numpy_num_den(self.counts, self.ni, genotype)
        return quantum(num, den_a[:, None], den_b[None, :])

    def block(self, a0, na, b0, nb):
        n11, gg, c, het, hom = self.counts[:5]
        ra, rb = slice(a0 - self.s0, a0 - self.s0 + na), slice(b0 - self.s0, b0 - self.s0 + nb)
        return n11[ra, rb], gg[ra, rb], c[ra], het[ra], hom[ra], c[rb], het[rb], hom[rb]

    def scores(self, snp_begin, win_lo, win_hi, genotype, q=None):
        """-> (score_q40 uint64, n_terms uint32) of SNPs snp_begin + t with windows [win_lo[t], win_hi[t]), all inside [s0, s0 + ns).
        q: other quanta than the truth's (self.quanta(genotype, another_form))"""
        q, poly = self.q[genotype] if q is None else q, self.poly[genotype]
        score = np.zeros(len(win_lo), dtype=np.uint64); terms = np.zeros(len(win_lo), dtype=np.uint32)
        for t, (lo, hi) in enumerate(zip(win_lo, win_hi)):
            assert self.s0 <= lo and hi <= self.s0 + self.ns
            score[t] = q[snp_begin + t - self.s0, int(lo) - self.s0:int(hi) - self.s0].sum(dtype=np.uint64)
            terms[t] = poly[int(lo) - self.s0:int(hi) - self.s0].sum()
        return score, terms

    def meaningful(self, snp_begin, win_lo, win_hi, genotype):
        """the conditions every score test asserts of its input: the windows hold a monomorphic and a polymorphic SNP, and some quantum
        is neither 0 nor 2^40"""
        q, poly = self.q[genotype], self.poly[genotype]
        lo, hi = int(min(win_lo)) - self.s0, int(max(win_hi)) - self.s0
        inside = np.concatenate([q[snp_begin + t - self.s0, int(a) - self.s0:int(b) - self.s0] for t, (a, b) in enumerate(zip(win_lo, win_hi))])
        return bool(poly[lo:hi].any() and (~poly[lo:hi]).any() and ((inside != 0) & (inside != np.uint64(1 << 40))).any())
