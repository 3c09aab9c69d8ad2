"""Shared by the score tests (test_ind_scores_cpu.py, test_gpu_ind_scores.py): the plain numpy statement of the per-individual scores --
the rows unpacked to a 0/1/2 matrix and an int64 matrix product, no words, no digits, no byte order -- and the weight columns that tell
a wrong byte order of the weight operand from a right one.  Everything is int64 and exact: the inputs keep |w| * 2 * n_snps far below
2^62."""
import numpy as np

from tests.snp_counts_inputs import random_rows

W_MAX = 1 << 30
# the digit-carry edges of the balanced base-256 split
EDGE_WEIGHTS = [0, 1, -1, 127, -127, 128, -128, 129, -129, 32768, -32768, W_MAX, -W_MAX]
NAMES = ("gscore", "hetscore")
# the population of the CPU test and, as founders of generation 0, of the GPU test: two slices of 4096 SNPs and 77
N_PEOPLE, L = 150, 2 * 4096 + 77
STEP = 256                                     # SNPs of a step of 4 words = byte positions of the four matrix steps of a lane group's word


def population_rows(seed=43):
    """150 people x 8269 SNPs with every allele frequency from 0 to 1, unpacked uint8 [300][8269]"""
    return random_rows(np.random.RandomState(seed), N_PEOPLE, L)


def genotypes(bits01):
    """unpacked haplotype rows [2 n][L] -> int64 [n][L] of 0/1/2"""
    return bits01[0::2].astype(np.int64) + bits01[1::2]


def numpy_scores(geno, s0, ns, i0, ni, w):
    """0/1/2 matrix [n][L], integer weights [n_scores][ns] -> (gscore, hetscore) int64 [n_scores][ni] of individuals [i0, +ni) over SNPs
    [s0, +ns)"""
    g = geno[i0:i0 + ni, s0:s0 + ns]
    w = np.atleast_2d(np.asarray(w, dtype=np.int64))
    assert w.shape[1] == ns and (w.size == 0 or int(np.abs(w).max()) * 2 * max(ns, 1) < 1 << 62)
    return w @ g.T, w @ (g == 1).T.astype(np.int64)


def one_hot_value(p):
    """a weight for byte position p of a step with a non-zero digit in each of the four places, signs mixed, different at every p < 256"""
    d0 = (1 + p % 127) * (-1 if p & 1 else 1)
    d1 = (3 + p % 100) * (-1 if p % 3 == 0 else 1)
    d2 = -(5 + p % 90) if p % 5 else 7 + p % 90
    d3 = (1 + p % 60) * (-1 if p & 2 else 1)
    return d0 + 256 * d1 + 65536 * d2 + 16777216 * d3


def one_hot_weights(n_snps, first=0, n_pos=STEP):
    """int32 [n_pos][n_snps]: column p is zero but for one_hot_value(p) at SNP first + p of the range, so that gscore[p][i] = g of
    individual i at that SNP times its value: every byte position of a step against every individual"""
    assert 0 <= first and first + n_pos <= n_snps
    vals = [one_hot_value(p) for p in range(n_pos)]
    assert len(set(vals)) == n_pos and all(abs(v) <= W_MAX for v in vals)
    w = np.zeros((n_pos, n_snps), dtype=np.int32)
    w[np.arange(n_pos), first + np.arange(n_pos)] = vals
    return w


def random_weights(rs, n_scores, n_snps):
    """int32 [n_scores][n_snps] over the whole range of a weight, the edges strewn in"""
    w = rs.randint(-W_MAX, W_MAX + 1, size=(n_scores, n_snps), dtype=np.int64)
    if w.size:
        at = rs.random_sample(w.shape) < 0.15
        w[at] = rs.choice(EDGE_WEIGHTS, size=int(at.sum()))
    return w.astype(np.int32)
