"""Shared by the pair count tests (test_pair_counts_cpu.py, test_gpu_pair_counts.py): the plain numpy statement of the counts."""
import numpy as np


def numpy_ind_counts(bits01, snp_begin=0, n_snps=None):
    """unpacked haplotype rows -> (n_het, n_hom_alt) per individual: rows 2i and 2i+1 paired, the SNPs of the range summed"""
    n_snps = bits01.shape[1] - snp_begin if n_snps is None else n_snps
    a, b = bits01[0::2, snp_begin:snp_begin + n_snps], bits01[1::2, snp_begin:snp_begin + n_snps]
    return (a ^ b).sum(axis=1, dtype=np.uint32), (a & b).sum(axis=1, dtype=np.uint32)


def numpy_pair_counts(bits01, snp_begin=0, n_snps=None, a_begin=0, n_a=None, b_begin=0, n_b=None, products=np.int64):
    """unpacked haplotype rows -> (n_hethet, n_opphom, dot) [n_a][n_b] in int64: x @ x.T, y @ z.T + z @ y.T, g @ g.T.  products: the type
    the matrix products are formed in -- np.float64 takes the BLAS route for a large population and is exact while every sum stays
    below 2^53 (a dot product is at most 4 n_snps)"""
    n_ind = bits01.shape[0] // 2
    n_snps = bits01.shape[1] - snp_begin if n_snps is None else n_snps
    n_a = n_ind - a_begin if n_a is None else n_a
    n_b = n_ind - b_begin if n_b is None else n_b
    h0 = bits01[0::2, snp_begin:snp_begin + n_snps].astype(np.int64); h1 = bits01[1::2, snp_begin:snp_begin + n_snps].astype(np.int64)
    x, y, z, g = ((h0 ^ h1).astype(products), (h0 & h1).astype(products), (1 - (h0 | h1)).astype(products), (h0 + h1).astype(products))
    ra, rb = slice(a_begin, a_begin + n_a), slice(b_begin, b_begin + n_b)
    return tuple(m.astype(np.int64) for m in (x[ra] @ x[rb].T, y[ra] @ z[rb].T + z[ra] @ y[rb].T, g[ra] @ g[rb].T))


class PairTruth:
    """the three n x n matrices and the two vectors of a whole population over one SNP range, computed once and sliced by the tests"""

    def __init__(self, bits01, snp_begin=0, n_snps=None, products=np.int64):
        self.het, self.hom = numpy_ind_counts(bits01, snp_begin, n_snps)
        self.hethet, self.opphom, self.dot = numpy_pair_counts(bits01, snp_begin, n_snps, products=products)

    def block(self, a_begin, n_a, b_begin, n_b):
        ra, rb = slice(a_begin, a_begin + n_a), slice(b_begin, b_begin + n_b)
        return self.hethet[ra, rb], self.opphom[ra, rb], self.dot[ra, rb]
