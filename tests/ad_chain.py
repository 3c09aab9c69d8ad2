"""Inputs for the tests of a generation's chain from the CV planes to A/D (tests/test_gpu_ad_chain.py, tests/test_ad_chain_cpu.py):
CV files in position order, one root population, so that the planes' column counts are added up behind the stitch and the wide
A/D kernel computes its terms from them.

New mutations are made to land on CV positions in every generation: the mutation map has rows that are ONE base pair wide
(bp[i - 1] == bp[i] == x: std::uniform_int_distribution(x, x) returns x) at chosen CV positions, with a rate close to 1, and the
first of them twice in a row, so that a task often hits that position twice.  Pure Python plus the oracle's kat_* helpers and the
scan arithmetic of tests/placed_hits.py."""
import numpy as np

from oracle import oracle_api
from tests import placed_hits as ph
from tests.synth import synth_packed  # noqa: F401 (tests take it from here)

R = 41
RBP = (1000 + 5000 * np.arange(R)).astype(np.uint64)         # the chromosome: [1000, 201000)
BP0, BP_END = int(RBP[0]), int(RBP[-1])
L = 256
SNPS = (1000 + 700 * np.arange(L)).astype(np.uint64)
HOT = 0.97
WIDE, FROM_COUNTS = 5, 16                                    # gev_dbg_ad_path


def cv_positions(ncv, uncovered=False):
    """ncv positions in file order == position order; uncovered: the last one lies behind the chromosome's end"""
    pos = (1500 + 150 * np.arange(ncv)).astype(np.uint64)
    assert int(pos[-1]) < BP_END
    if uncovered:
        pos[-1] = BP_END + 50
    return pos


def hot_positions(cvpos):
    """the CV positions the mutation map aims at: the first (twice), a middle one and the last covered one"""
    inside = [int(x) for x in cvpos if BP0 <= int(x) < BP_END]
    return sorted({inside[0], inside[len(inside) // 2], inside[-1]})


def mutation_map(hot, background=0.01):
    """rows: [.., x] wide (background rate), [x, x] one base pair (HOT); the first hot position has two such rows.
    -> (bp, rate, {row: x} of the one-base-pair rows)"""
    bp, rate, rows = [BP0], [0.0], {}
    for i, x in enumerate(hot):
        bp.append(x); rate.append(background)
        for _ in range(2 if i == 0 else 1):
            rows[len(bp)] = x
            bp.append(x); rate.append(HOT)
    bp.append(BP_END - 1); rate.append(background)
    return np.array(bp, dtype=np.uint64), np.array(rate), rows


class Case:
    """static inputs of one context: per chromosome a list over phenotypes of (CV positions, a, d, vd)"""

    def __init__(self, n_ind, ncv, vd=(0.0,), nchr=1, with_mut=True, uncovered=False, seed=5, rec=0.03):
        self.n_ind, self.nchr, self.nphen, self.with_mut = n_ind, nchr, len(vd), with_mut
        self.rprob = np.r_[0.0, np.full(R - 1, rec)]
        ncv = np.broadcast_to(np.asarray(ncv), (self.nphen, nchr)) if np.ndim(ncv) else np.full((self.nphen, nchr), ncv)
        rs = np.random.RandomState(seed)
        self.cv = [[(cv_positions(int(ncv[p][c]), uncovered and int(ncv[p][c]) > 1), rs.randn(int(ncv[p][c])), 0.3 * rs.randn(int(ncv[p][c])), vd[p])
                    for c in range(nchr)] for p in range(self.nphen)]
        # the mutation map of a chromosome aims at the CV positions of phenotype 0 there
        self.mmap = [mutation_map(hot_positions(self.cv[0][c][0])) for c in range(nchr)]

    def apply(self, ctx):
        nh = 2 * self.n_ind
        for c in range(self.nchr):
            ctx.set_rmap(0, c, RBP, self.rprob, 5000)
            if self.with_mut:
                ctx.set_mutmap(0, c, self.mmap[c][0], self.mmap[c][1])
            ctx.set_snps(0, c, SNPS)
            for p in range(self.nphen):
                ctx.set_cvs(0, p, c, *self.cv[p][c])
        for c in range(self.nchr):
            ctx.upload_founders(0, c, synth_packed(11 + c, nh, L), L)
            for p in range(self.nphen):
                n = len(self.cv[p][c][0])
                ctx.upload_cv_founders(0, p, c, synth_packed(31 + 7 * p + c, nh, n), n)

    def couples(self, n=None):
        n = self.n_ind if n is None else n
        return np.array([(i, (i + 1) % n, 0, 1) for i in range(n)], dtype=np.int64)

    def mut_seeds(self, gen):
        return (1000 * gen + 17 * np.arange(self.n_ind * self.nchr)).astype(np.uint32)

    def predicted_hits(self, ol, gen):
        """the new mutations of every task of a gev_reproduce with mut_seeds(gen) on the one-base-pair rows, from the scan arithmetic
        alone: {task: [(position, side)] in hit order} (hits on the wide rows are left out: their positions are drawn)"""
        out = {}
        for t, S in enumerate(self.mut_seeds(gen)):
            bp, rate, hot_rows = self.mmap[t % self.nchr]
            rows = ph.scan(ol, int(S) + 2, 1, rate, len(bp) - 1)
            r = oracle_api.kat_rand(ol, int(S), len(rows) + 2)
            out[t] = [(hot_rows[row], int(r[h]) % 2) for h, row in enumerate(rows) if row in hot_rows]
        return out


def repeated_hits(hits):
    """tasks that hit one position twice on the same haplotype: [(task, position, side)]"""
    return [(t, x, s) for t, hs in hits.items() for x, s in set(hs) if hs.count((x, s)) >= 2]
