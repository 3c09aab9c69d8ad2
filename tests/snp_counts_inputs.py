"""Shared by the genotype count tests (test_snp_counts_cpu.py, test_gpu_snp_counts.py): the overflow period of the counter as built, random
rows with every allele frequency, and the plain numpy statement of the counts."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counter_period():
    """F = 2^K - 1 of the counter as built (GEV_SNPC_K of the header)"""
    src = open(os.path.join(ROOT, "geneevolve_amd", "csrc", "gev_snpcount.h")).read()
    return (1 << int(re.search(r"#define\s+GEV_SNPC_K\s+(\d+)", src).group(1))) - 1


F = counter_period()


def random_rows(rs, n_ind, L):
    """uint8 [2 * n_ind][L] of 0/1 with per-SNP frequencies from 0 to 1: column 0 all zero, the last column all one (L >= 2)"""
    f = rs.permutation(np.linspace(0.0, 1.0, L)) if L > 2 else np.array([0.0, 1.0][:L])
    if L >= 2:
        f[0], f[-1] = 0.0, 1.0
    return (rs.random_sample((2 * n_ind, L)) < f).astype(np.uint8)


def numpy_counts(bits01, snp_begin=0, n_snps=None):
    """unpacked haplotype rows -> (n_het, n_hom_alt): rows 2i and 2i+1 paired, columns summed"""
    n_snps = bits01.shape[1] - snp_begin if n_snps is None else n_snps
    a, b = bits01[0::2, snp_begin:snp_begin + n_snps], bits01[1::2, snp_begin:snp_begin + n_snps]
    return (a ^ b).sum(axis=0, dtype=np.uint32), (a & b).sum(axis=0, dtype=np.uint32)
