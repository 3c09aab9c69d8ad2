"""Linkage disequilibrium from the device's SNP-pair counts (GevContext.ld_counts / ld_scores): haplotype r^2, D', genotype r^2 between two
ranges of SNPs of one population -- of one chromosome or of two -- and LD scores over windows given by count or by map distance.
Nothing is downloaded but the integer matrices, or for LD scores two vectors; every statistic is formed from exact integers in float64."""
from collections import namedtuple

import numpy as np

from ._ranges import individuals as _range

Q40 = float(1 << 40)

LDCounts = namedtuple("LDCounts", "n_ind n11 gg c_a het_a hom_a c_b het_b hom_b")
LDCounts.__doc__ = """n_ind: individuals counted (N; n = 2 N haplotypes); n11 / gg: int64 [n_a][n_b] per pair (SNP j of a, SNP k of b): haplotypes with
allele 1 at both, sum_i g_ij g_ik; c_* / het_* / hom_*: int64 [n_a] / [n_b] allele-1 count, heterozygous and homozygous-alt individuals per SNP"""

LDScores = namedtuple("LDScores", "score n_terms adjusted score_q40")
LDScores.__doc__ = """score: float64 [n_snps] = score_q40 / 2^40, the sum of r^2 over each SNP's window (itself included); n_terms: the window's SNPs that
are polymorphic among the individuals; adjusted: the sum of LDSC's r^2 - (1 - r^2) / (n - 2) over them = score - (n_terms - score) / (n - 2),
n = the haplotypes (haplotype r^2) or individuals (genotype r^2) counted; score_q40: the exact integers (uint64)"""


def counts(ctx, pop, chr_a, a=None, chr_b=None, b=None, ind=None):
    """the counts of SNP pairs (j of a on chr_a, k of b on chr_b) over the individuals `ind`; a, b, ind: None (all) or (begin, n)"""
    chr_b = chr_a if chr_b is None else chr_b
    a0, na = (0, ctx._nsnp[(pop, chr_a)]) if a is None else _range(ctx, pop, a)
    b0, nb = (0, ctx._nsnp[(pop, chr_b)]) if b is None else _range(ctx, pop, b)
    i0, ni = _range(ctx, pop, ind)
    out = ctx.ld_counts(pop, chr_a, a0, na, chr_b, b0, nb, i0, ni)
    return LDCounts(ni, *(x.astype(np.int64) for x in out))


def _num_den(ld, genotype):
    n = ld.n_ind if genotype else 2 * ld.n_ind
    num = n * (ld.gg if genotype else ld.n11) - ld.c_a[:, None] * ld.c_b[None, :]
    if genotype:
        den_a = n * (ld.het_a + 4 * ld.hom_a) - ld.c_a * ld.c_a; den_b = n * (ld.het_b + 4 * ld.hom_b) - ld.c_b * ld.c_b
    else:
        den_a = ld.c_a * (n - ld.c_a); den_b = ld.c_b * (n - ld.c_b)
    return num, den_a, den_b


def _r2(ld, genotype):
    num, den_a, den_b = _num_den(ld, genotype)
    x = num.astype(np.float64)
    den = den_a.astype(np.float64)[:, None] * den_b.astype(np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, (x * x) / den, np.nan)


def r2_haplotype(ld):
    """float64 [n_a][n_b]: (n n11 - c_j c_k)^2 / (c_j (n - c_j) c_k (n - c_k)); NaN where a SNP is monomorphic"""
    return _r2(ld, False)


def r2_genotype(ld):
    """float64 [n_a][n_b]: the squared correlation of the genotypes (0/1/2), (N gg - s_j s_k)^2 / ((N sum g_j^2 - s_j^2)(N sum g_k^2 - s_k^2));
    NaN where a SNP is monomorphic"""
    return _r2(ld, True)


def d_prime(ld):
    """float64 [n_a][n_b]: Lewontin's D' with its sign, D / D_max with D = n11 / n - p_j p_k and D_max = min(p_j (1 - p_k), (1 - p_j) p_k)
    for D > 0, min(p_j p_k, (1 - p_j)(1 - p_k)) for D < 0; NaN where a SNP is monomorphic"""
    n = 2 * ld.n_ind
    num = n * ld.n11 - ld.c_a[:, None] * ld.c_b[None, :]                  # n^2 D
    ca, cb = ld.c_a[:, None], ld.c_b[None, :]
    dmax = np.where(num >= 0, np.minimum(ca * (n - cb), (n - ca) * cb), np.minimum(ca * cb, (n - ca) * (n - cb)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(dmax > 0, num.astype(np.float64) / dmax.astype(np.float64), np.nan)


def windows_by_count(L, snp_begin, n_snps, w):
    """(win_lo, win_hi), uint32 [n_snps]: for SNP j = snp_begin + t the SNPs [j - w, j + w] of a chromosome of L SNPs"""
    j = np.arange(snp_begin, snp_begin + n_snps, dtype=np.int64)
    return np.maximum(j - int(w), 0).astype(np.uint32), np.minimum(j + int(w) + 1, L).astype(np.uint32)


def windows_by_distance(pos, snp_begin, n_snps, max_dist):
    """(win_lo, win_hi), uint32 [n_snps]: for SNP j = snp_begin + t the SNPs k with |pos[k] - pos[j]| <= max_dist; pos: the chromosome's
    non-decreasing positions in any unit (base pairs, cM)"""
    pos = np.asarray(pos)
    pos = pos.astype(np.float64) if pos.dtype.kind == "f" else pos.astype(np.int64)
    assert (pos[1:] >= pos[:-1]).all(), "positions in map order"
    mine = pos[snp_begin:snp_begin + n_snps]
    return np.searchsorted(pos, mine - max_dist, side="left").astype(np.uint32), np.searchsorted(pos, mine + max_dist, side="right").astype(np.uint32)


def ld_scores(ctx, pop, chr, win_lo=None, win_hi=None, w=None, snp_begin=0, n_snps=None, ind=None, genotype=False):
    """LD scores of SNPs [snp_begin, +n_snps) of (pop, chr) over the individuals `ind` (None or (begin, n)), the windows given as the two
    arrays or as a count w of SNPs to either side -> LDScores"""
    L = ctx._nsnp[(pop, chr)]
    n_snps = L - snp_begin if n_snps is None else n_snps
    if win_lo is None:
        assert w is not None and win_hi is None, "windows: two arrays, or a count"
        win_lo, win_hi = windows_by_count(L, snp_begin, n_snps, w)
    i0, ni = _range(ctx, pop, ind)
    q, terms = ctx.ld_scores(pop, chr, win_lo, win_hi, snp_begin, n_snps, i0, ni, genotype)
    score = q.astype(np.float64) / Q40
    n = ni if genotype else 2 * ni
    with np.errstate(divide="ignore", invalid="ignore"):
        adjusted = score - (terms - score) / (n - 2.0) if n != 2 else np.full_like(score, np.nan)
    return LDScores(score, terms, adjusted, q)
