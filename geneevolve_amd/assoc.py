"""Association of traits with every SNP from the device's per-SNP trait sums (GevContext.snp_trait_sums): the additive regression and
the genotypic (2-df) test of one population's current generation.  Nothing is downloaded but the integer sums, two int64 per SNP and
trait and two counts per SNP.  A floating-point phenotype is quantised to int32 first, so the sums are exact integers; every statistic
is formed from them exactly in Python integers (object arrays) as far as it cancels and converted to float64 once.  p-values are left
to the caller."""
from collections import namedtuple

import numpy as np

from ._ranges import individuals as _range
from .scores import quantise_weights

TraitSums = namedtuple("TraitSums", "n_ind gsum hetsum n_het n_hom_alt sum_q sum_q2 scale mean")
TraitSums.__doc__ = """n_ind: individuals summed over (N); gsum / hetsum: int64 [n_traits][n_snps], sum_i g_ij q[t][i] and the sum of q[t][i] over the
heterozygous individuals; n_het / n_hom_alt: int64 [n_snps]; sum_q / sum_q2: per trait sum q and sum q^2 (Python integers, object [n_traits]);
scale / mean: float64 [n_traits], y = q * scale + mean (1 and 0 for a trait given as quanta)"""

Additive = namedtuple("Additive", "beta se t r2")
Additive.__doc__ = """float64 [n_traits][n_snps] of the regression of the trait on g = 0/1/2: slope (in the units of y per allele), its standard error
(residual variance on N - 2 degrees of freedom), t = beta / se, and the squared correlation; NaN where the SNP is monomorphic among the
individuals, and for se / t / r2 where they are not defined (a constant trait, N <= 2)"""

Genotypic = namedtuple("Genotypic", "means F df1 df2")
Genotypic.__doc__ = """means: float64 [3][n_traits][n_snps], the trait's mean (in the units of y) in the genotype classes 0/0, 0/1, 1/1, NaN for an empty
class; F: float64 [n_traits][n_snps], the one-way F statistic between the classes, on df1 = (non-empty classes - 1) and df2 = N - non-empty
classes degrees of freedom (int64 [n_snps]): the 2-df genotypic test where all three classes are present; NaN where the SNP is monomorphic
or df2 < 1 or the trait is constant"""


def quantise(y, bits=30):
    """float phenotypes [n_traits][n_ind] (or [n_ind]) -> (q int32, scale float64 [n_traits], mean float64 [n_traits]): centred on the mean over the
    individuals given, then scaled and rounded as scores.quantise_weights does, so |q * scale + mean - y| <= scale / 2"""
    assert 1 <= bits <= 30
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    if y.shape[1] == 0:
        return np.zeros(y.shape, dtype=np.int32), np.ones(y.shape[0]), np.zeros(y.shape[0])
    mean = y.mean(axis=1)
    return (*quantise_weights(y - mean[:, None], bits), mean)


def _exact_moments(q):
    """per trait (sum q, sum q^2) as Python integers; q^2 summed in three int64 limbs of 16-bit halves, each below 2^63 for 2^22 individuals"""
    q = q.astype(np.int64)
    lo, hi = q & 0xFFFF, q >> 16
    s = [int(v) for v in q.sum(axis=1)]
    s2 = [(int(a) << 32) + (int(b) << 17) + int(c) for a, b, c in zip((hi * hi).sum(axis=1), (hi * lo).sum(axis=1), (lo * lo).sum(axis=1))]
    return np.array(s, dtype=object), np.array(s2, dtype=object)


def sums(ctx, pop, chr, y_or_q, snps=None, ind=None):
    """the trait sums of SNPs `snps` of (pop, chr) over the individuals `ind` (each None: all, or (begin, n)).  y_or_q: [n_traits][n_ind] or
    [n_ind], entry i = individual begin + i; an integer array is taken as int32 quanta (|q| <= 2^30), a floating-point one is quantised
    (quantise) -> TraitSums"""
    s0, ns = (0, ctx._nsnp[(pop, chr)]) if snps is None else _range(ctx, pop, snps)
    i0, ni = _range(ctx, pop, ind)
    y = np.atleast_2d(np.asarray(y_or_q))
    assert y.shape[1] == ni, "one value per trait and individual of the range"
    if y.dtype.kind in "iu":
        assert y.size == 0 or np.abs(y.astype(np.int64)).max() <= 1 << 30, "quanta beyond +-2^30"
        q, scale, mean = y.astype(np.int32), np.ones(y.shape[0]), np.zeros(y.shape[0])
    else:
        q, scale, mean = quantise(y)
    gsum, hetsum, het, hom = ctx.snp_trait_sums(pop, chr, q, s0, ns, i0, ni)
    sq, sq2 = _exact_moments(q)
    return TraitSums(ni, gsum, hetsum, het.astype(np.int64), hom.astype(np.int64), sq, sq2, scale, mean)


def _ratio(num, den, ok):
    """float64 of the exact quotient num / den of two object arrays of Python integers (one correctly rounded conversion) where ok, NaN elsewhere"""
    num, den, ok = np.broadcast_arrays(num, den, ok)
    out = np.full(num.shape, np.nan)
    if ok.any():
        out[ok] = (num[ok] / den[ok]).astype(np.float64)
    return out


def additive(s):
    """the regression of every trait on the allele count of every SNP -> Additive.  With c = sum g, N sum g q - c sum q cancels and
    exceeds int64 at large N, so it and the other cancelling terms are formed in Python integers before the one conversion to double"""
    N = int(s.n_ind)
    c = (s.n_het + 2 * s.n_hom_alt).astype(object)[None, :]
    den_g = N * (s.n_het + 4 * s.n_hom_alt).astype(object)[None, :] - c * c                      # N sum g^2 - (sum g)^2
    den_q = (N * s.sum_q2 - s.sum_q * s.sum_q)[:, None]                                           # N sum q^2 - (sum q)^2
    num = N * s.gsum.astype(object) - c * s.sum_q[:, None]
    rest = den_q * den_g - num * num                                                              # N^2 den_g times the residual sum of squares
    poly = den_g > 0
    scale = s.scale[:, None]
    beta = _ratio(num, den_g, poly) * scale
    ok = poly & (N > 2)
    se = np.sqrt(_ratio(rest, (N - 2) * den_g * den_g, ok)) * scale
    t = np.sign(_ratio(num, den_g, ok)) * np.sqrt(_ratio(num * num * (N - 2), rest, ok & (rest > 0)))
    r2 = _ratio(num * num, den_g * den_q, poly & (den_q > 0))
    return Additive(beta, se, t, r2)


def genotypic(s):
    """the trait's mean per genotype class and the one-way F statistic between the classes -> Genotypic.  The class sums are S1 = hetsum,
    S2 = (gsum - hetsum) / 2, S0 = sum q - S1 - S2; the sums of squares are formed over the common denominator N n0 n1 n2 in Python integers"""
    N = int(s.n_ind)
    n = [(N - s.n_het - s.n_hom_alt).astype(object)[None, :], s.n_het.astype(object)[None, :], s.n_hom_alt.astype(object)[None, :]]
    S1 = s.hetsum.astype(object); S2 = (s.gsum.astype(object) - S1) // 2; S0 = s.sum_q[:, None] - S1 - S2
    S = [S0, S1, S2]
    means = np.stack([_ratio(S[k], n[k], n[k] > 0) * s.scale[:, None] + s.mean[:, None] for k in range(3)])
    if N == 0:
        z = np.zeros(s.n_het.shape, dtype=np.int64)
        return Genotypic(means, np.full(s.gsum.shape, np.nan), z - 1, z)
    m = [np.where(n[k] > 0, n[k], 1) for k in range(3)]                                           # an empty class: factor 1, its sum is 0
    D = N * m[0] * m[1] * m[2]
    sq = s.sum_q[:, None]
    ssb = sum(S[k] * S[k] * (D // m[k]) for k in range(3)) - sq * sq * (D // N)                   # D times the between-class sum of squares
    ssw = (N * s.sum_q2[:, None] - sq * sq) * (D // N) - ssb                                      # D times the within-class one
    classes = sum((n[k] > 0).astype(np.int64) for k in range(3))[0]
    df1, df2 = classes - 1, N - classes
    F = _ratio(ssb * df2.astype(object)[None, :], ssw * df1.astype(object)[None, :], (df1 > 0)[None, :] & (df2 > 0)[None, :] & (ssw > 0))
    return Genotypic(means, F, df1, df2)
