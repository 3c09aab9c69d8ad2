"""Relatedness from the device's pairwise genotype counts (GevContext.pair_genotype_counts / ind_genotype_counts): IBS distance, KING
kinship and a VanRaden GRM between two ranges of individuals of one population, summed over the context's active chromosomes.
Nothing is downloaded but the integer matrices; every statistic is formed from exact integers in float64."""
from collections import namedtuple

import numpy as np

from ._ranges import individuals as _range

PairCounts = namedtuple("PairCounts", "n_snps het_a hom_a het_b hom_b n_hethet n_opphom dot")
PairCounts.__doc__ = """n_snps: loci counted; het_* / hom_*: int64 [n_a] / [n_b] heterozygous loci and loci with allele 1 twice of each individual;
n_hethet / n_opphom / dot: int64 [n_a][n_b] per pair (i of a, k of b)"""


def pair_counts(ctx, pop, a=None, b=None):
    """the counts of pairs (i of a, k of b) summed over the active chromosomes; a, b: None (the whole population) or (begin, n)"""
    a0, na = _range(ctx, pop, a); b0, nb = _range(ctx, pop, b)
    het_a = np.zeros(na, dtype=np.int64); hom_a = np.zeros(na, dtype=np.int64)
    het_b = np.zeros(nb, dtype=np.int64); hom_b = np.zeros(nb, dtype=np.int64)
    mats = [np.zeros((na, nb), dtype=np.int64) for _ in range(3)]
    n_snps = 0
    for chr in ctx.active_chrs():
        n_snps += ctx._nsnp[(pop, chr)]
        h, m = ctx.ind_genotype_counts(pop, chr, ind_begin=a0, n_ind=na); het_a += h; hom_a += m
        h, m = (h, m) if (a0, na) == (b0, nb) else ctx.ind_genotype_counts(pop, chr, ind_begin=b0, n_ind=nb); het_b += h; hom_b += m
        for acc, part in zip(mats, ctx.pair_genotype_counts(pop, chr, a_begin=a0, n_a=na, b_begin=b0, n_b=nb)):
            acc += part
    return PairCounts(n_snps, het_a, hom_a, het_b, hom_b, *mats)


def ibs_distance(pc):
    """int64 [n_a][n_b]: sum_j |g_ij - g_kj| = het_i + het_k - 2 n_hethet + 2 n_opphom"""
    return pc.het_a[:, None] + pc.het_b[None, :] - 2 * pc.n_hethet + 2 * pc.n_opphom


def king_kinship(pc, robust=False):
    """float64 [n_a][n_b]: the KING kinship estimate; homogeneous: (n_hethet - 2 n_opphom) / (het_i + het_k); robust, with m = min(het_i,
    het_k): (n_hethet - 2 n_opphom) / (2 m) + 1/2 - (het_i + het_k) / (4 m).  NaN where the denominator is 0"""
    num = (pc.n_hethet - 2 * pc.n_opphom).astype(np.float64)
    hs = (pc.het_a[:, None] + pc.het_b[None, :]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if not robust:
            return np.where(hs > 0, num / hs, np.nan)
        m = np.minimum(pc.het_a[:, None], pc.het_b[None, :]).astype(np.float64)
        return np.where(m > 0, num / (2.0 * m) + 0.5 - hs / (4.0 * m), np.nan)


def grm_from_counts(dot, s_a, s_b, sum_c2, sum_c_2n_minus_c, n_pop):
    """the VanRaden GRM from exact integers: dot int64 [n_a][n_b]; s_* = sum_j c_j g_ij; sum_c2 = sum c_j^2, sum_c_2n_minus_c = sum c_j (2N - c_j)
    (Python integers), c_j = the allele-1 count of SNP j among the N individuals.  With p_j = c_j / 2N and z_ij = g_ij - 2 p_j:
        Z Z' = dot - (s_i + s_k) / N + sum c_j^2 / N^2          sum_j 2 p_j (1 - p_j) = sum c_j (2N - c_j) / (2 N^2)"""
    n = float(n_pop)
    zz = dot.astype(np.float64) - (s_a[:, None] + s_b[None, :]).astype(np.float64) / n + float(sum_c2) / (n * n)
    den = float(sum_c_2n_minus_c) / (2.0 * n * n)
    with np.errstate(divide="ignore", invalid="ignore"):
        return zz / den if den > 0 else np.full_like(zz, np.nan)


def grm_vanraden(ctx, pop, a=None, b=None):
    """float64 [n_a][n_b]: VanRaden's first GRM, Z Z' / sum 2 p (1 - p), allele frequencies from the whole population (snp_genotype_counts)"""
    a0, na = _range(ctx, pop, a); b0, nb = _range(ctx, pop, b)
    n_pop = ctx.pop_size(pop)
    dot = np.zeros((na, nb), dtype=np.int64)
    s_a = np.zeros(na, dtype=np.uint64); s_b = np.zeros(nb, dtype=np.uint64)
    sum_c2 = 0; sum_cc = 0
    for chr in ctx.active_chrs():
        het, hom = ctx.snp_genotype_counts(pop, chr)
        c = het + 2 * hom                                       # uint32: at most 2 N
        ci = c.astype(object)
        sum_c2 += int((ci * ci).sum()); sum_cc += int((ci * (2 * n_pop - ci)).sum())
        s = ctx.ind_genotype_counts(pop, chr, ind_begin=a0, n_ind=na, weight=c)[2]; s_a += s
        s_b += s if (a0, na) == (b0, nb) else ctx.ind_genotype_counts(pop, chr, ind_begin=b0, n_ind=nb, weight=c)[2]
        dot += ctx.pair_genotype_counts(pop, chr, a_begin=a0, n_a=na, b_begin=b0, n_b=nb)[2]
    return grm_from_counts(dot, s_a, s_b, sum_c2, sum_cc, n_pop)
