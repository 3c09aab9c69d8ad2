"""Shared by the pair count tests (test_pair_counts_cpu.py, test_gpu_pair_counts.py): the plain numpy statement of the counts; and, with
the LD tests, the tile mode of the matrix-core product both run on."""
import numpy as np


class tile_mode:
    """with tile_mode(ctx, mode) as t: the products of the calls inside run under gev_dbg_bitprod_tiles(mode) (0 = tiles by compute
    units, 1 = always 64 x 64, 2 = always 128 x 128); t.launched() = (small, large) product launches since the block was entered, and
    since the last t.launched().  The mode is 0 again afterwards, whatever happened inside"""

    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        self.seen = self.ctx.dbg_bitprod_tiles(self.mode)
        return self

    def launched(self):
        now = self.ctx.dbg_bitprod_tiles()
        delta = (now[0] - self.seen[0], now[1] - self.seen[1])
        self.seen = now
        return delta

    def large_only(self):
        """every product launch since the last look was on tiles of 128 x 128, and there was one"""
        small, large = self.launched()
        return small == 0 and large > 0

    def __exit__(self, *exc):
        self.ctx.dbg_bitprod_tiles(0)
        return False


def numpy_ind_counts(bits01, snp_begin=0, n_snps=None):
    """unpacked haplotype rows -> (n_het, n_hom_alt) per individual: rows 2i and 2i+1 paired, the SNPs of the range summed"""
    n_snps = bits01.shape[1] - snp_begin if n_snps is None else n_snps
    a, b = bits01[0::2, snp_begin:snp_begin + n_snps], bits01[1::2, snp_begin:snp_begin + n_snps]
    return (a ^ b).sum(axis=1, dtype=np.uint32), (a & b).sum(axis=1, dtype=np.uint32)


def numpy_pair_counts(bits01, snp_begin=0, n_snps=None, a_begin=0, n_a=None, b_begin=0, n_b=None, products=np.int64, only=None):
    """unpacked haplotype rows -> (n_hethet, n_opphom, dot) [n_a][n_b] in int64: x @ x.T, y @ z.T + z @ y.T, g @ g.T.  products: the type
    the matrix products are formed in -- np.float64 takes the BLAS route for a large population and is exact while every sum stays
    below 2^53 (a dot product is at most 4 n_snps).  only = 0, 1, 2: that matrix alone, not a tuple (a block of thousands a side, one
    matrix at a time)"""
    n_ind = bits01.shape[0] // 2
    n_snps = bits01.shape[1] - snp_begin if n_snps is None else n_snps
    n_a = n_ind - a_begin if n_a is None else n_a
    n_b = n_ind - b_begin if n_b is None else n_b
    h0 = bits01[0::2, snp_begin:snp_begin + n_snps].astype(np.int64); h1 = bits01[1::2, snp_begin:snp_begin + n_snps].astype(np.int64)
    x, y, z, g = ((h0 ^ h1).astype(products), (h0 & h1).astype(products), (1 - (h0 | h1)).astype(products), (h0 + h1).astype(products))
    ra, rb = slice(a_begin, a_begin + n_a), slice(b_begin, b_begin + n_b)
    matrices = (lambda: x[ra] @ x[rb].T, lambda: y[ra] @ z[rb].T + z[ra] @ y[rb].T, lambda: g[ra] @ g[rb].T)
    if only is not None:
        return matrices[only]().astype(np.int64)
    return tuple(m().astype(np.int64) for m in matrices)


class PairTruth:
    """the three n x n matrices and the two vectors of a whole population over one SNP range, computed once and sliced by the tests"""

    def __init__(self, bits01, snp_begin=0, n_snps=None, products=np.int64):
        self.het, self.hom = numpy_ind_counts(bits01, snp_begin, n_snps)
        self.hethet, self.opphom, self.dot = numpy_pair_counts(bits01, snp_begin, n_snps, products=products)

    def block(self, a_begin, n_a, b_begin, n_b):
        ra, rb = slice(a_begin, a_begin + n_a), slice(b_begin, b_begin + n_b)
        return self.hethet[ra, rb], self.opphom[ra, rb], self.dot[ra, rb]
