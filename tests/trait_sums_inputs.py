"""Shared by the trait-sum tests (test_trait_sums_cpu.py, test_gpu_trait_sums.py): the plain numpy statement of the per-SNP trait sums and
the traits that tell a wrong byte order of the trait operand from a right one.  Everything is int64 and exact: the inputs keep
|q| * n_ind far below 2^62."""
import numpy as np

Q_MAX = 1 << 30
# the digit-carry edges of the balanced base-256 split
EDGE_QUANTA = [Q_MAX, -Q_MAX, 0, 1, -1, 127, -127, 128, -128, 129, -129, 32768, -32768, 32767, -32769, 8388608, -8388608, 8388607, (1 << 30) - 1, 1 - (1 << 30)]
NAMES = ("gsum", "hetsum", "n_het", "n_hom_alt")


def numpy_trait_sums(bits01, s0, ns, i0, ni, q):
    """unpacked haplotype rows, int quanta [n_traits][ni] -> (gsum, hetsum int64 [n_traits][ns], n_het, n_hom_alt int64 [ns]) of SNPs [s0, +ns)
    over individuals [i0, +ni)"""
    h = bits01[2 * i0:2 * (i0 + ni), s0:s0 + ns].astype(np.int64)
    g = h[0::2] + h[1::2]
    q = np.atleast_2d(np.asarray(q, dtype=np.int64))
    assert q.shape[1] == ni and (q.size == 0 or int(np.abs(q).max()) * max(ni, 1) < 1 << 62)
    return q @ g, q @ (g == 1).astype(np.int64), (g == 1).sum(axis=0), (g == 2).sum(axis=0)


def one_hot_value(p):
    """a quantum for position p with a non-zero digit in each of the four places, signs mixed, different at every p < 128"""
    d0 = (1 + p % 120) * (-1 if p & 1 else 1)
    d1 = (3 + p % 100) * (-1 if p % 3 == 0 else 1)
    d2 = -(5 + p % 90) if p % 5 else 7 + p % 90
    d3 = (1 + p % 60) * (-1 if p & 2 else 1)
    return d0 + 256 * d1 + 65536 * d2 + 16777216 * d3


def one_hot_traits(n_ind, first=0, n_pos=128):
    """int32 [n_pos][n_ind]: trait p is zero but for one_hot_value(p) at individual first + p of the range, so that gsum[p][j] = g_j of that
    individual times its value: every individual position of a 128-individual matrix step against every SNP"""
    assert first + n_pos <= n_ind
    vals = [one_hot_value(p) for p in range(n_pos)]
    assert len(set(vals)) == n_pos and all(abs(v) <= Q_MAX for v in vals)
    q = np.zeros((n_pos, n_ind), dtype=np.int32)
    q[np.arange(n_pos), first + np.arange(n_pos)] = vals
    return q


def random_quanta(rs, n_traits, n_ind):
    """int32 [n_traits][n_ind] over the whole range of a quantum, the edges strewn in"""
    q = rs.randint(-Q_MAX, Q_MAX + 1, size=(n_traits, n_ind), dtype=np.int64)
    if q.size:
        at = rs.random_sample(q.shape) < 0.15
        q[at] = rs.choice(EDGE_QUANTA, size=int(at.sum()))
    return q.astype(np.int32)
