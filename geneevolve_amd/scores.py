"""Polygenic scores of one population's current generation from the device's per-individual scores (GevContext.ind_scores): signed
weight columns against the genotypes, G W, several dozen columns in one pass.  Nothing is downloaded but the integer sums, two int64
per individual and column.  Floating-point effect sizes are quantised to int32 first, so the sums are exact integers, additive over
SNP ranges and chromosomes and the same in every order; they are converted to float64 once, at the end."""
import numpy as np

from ._ranges import individuals as _individuals

MAX_SNPS = 1 << 22        # SNPs of one gev_ind_scores call (a digit's sum is an int32): longer ranges are split here and added


def quantise_weights(beta, bits=30):
    """float effect sizes [n_scores][n_snps] (or [n_snps]) -> (q int32, scale float64 [n_scores]): not centred (a score is linear in its
    weights, a constant would add a multiple of the allele count), scaled per column so that max |beta| maps to 2^bits and rounded to
    nearest, so |q * scale - beta| <= scale / 2.  A column of zeros gets scale 1"""
    assert 1 <= bits <= 30
    beta = np.atleast_2d(np.asarray(beta, dtype=np.float64))
    top = np.abs(beta).max(axis=1) if beta.shape[1] else np.zeros(beta.shape[0])
    scale = np.where(top > 0, top / float(1 << bits), 1.0)
    q = np.clip(np.rint(beta / scale[:, None]), -(1 << bits), 1 << bits).astype(np.int32)
    return q, scale


def sums(ctx, pop, weights_by_chr, ind=None, want=(True, True)):
    """the integer scores of the individuals `ind` (None: everybody, or (begin, n)) summed over the chromosomes of weights_by_chr, a dict
    chr -> int32 q[n_scores][L of that chromosome] (|q| <= 2^30; the same n_scores on every chromosome) -> (gscore, hetscore), int64
    [n_scores][n_ind], None where not wanted.  |sum| must stay below 2^63: 2^53 per call of at most 2^22 SNPs, so a thousand full calls"""
    i0, ni = _individuals(ctx, pop, ind)
    total = None
    for chr in sorted(weights_by_chr):
        q = np.atleast_2d(np.asarray(weights_by_chr[chr]))
        assert q.dtype.kind in "iu" and q.shape[1] == ctx._nsnp[(pop, chr)], "one integer weight per column and SNP of the chromosome"
        assert q.size == 0 or np.abs(q.astype(np.int64)).max() <= 1 << 30, "weights beyond +-2^30"
        if total is None:
            total = [np.zeros((q.shape[0], ni), dtype=np.int64) if w else None for w in want]
        assert all(t is None or t.shape[0] == q.shape[0] for t in total), "the same columns on every chromosome"
        for s0 in range(0, q.shape[1], MAX_SNPS):
            ns = min(MAX_SNPS, q.shape[1] - s0)
            part = ctx.ind_scores(pop, chr, np.ascontiguousarray(q[:, s0:s0 + ns], dtype=np.int32), s0, ns, i0, ni, want=want)
            for t, p in zip(total, part):
                if t is not None:
                    t += p
    if total is None:
        total = [np.zeros((0, ni), dtype=np.int64) if w else None for w in want]
    return tuple(total)


def prs(ctx, pop, beta_by_chr, ind=None, dominance_by_chr=None):
    """polygenic scores -> float64 [n_scores][n_ind]: sum_j beta[s][j] g_ij over the chromosomes of beta_by_chr (chr -> float
    [n_scores][L]), plus with dominance_by_chr (the same shape) sum_j delta[s][j] [i heterozygous at j].  A column is quantised with one
    scale over all its chromosomes, so the integer sums add before the one multiplication"""
    def quantised(by_chr):
        chrs = sorted(by_chr)
        beta = [np.atleast_2d(np.asarray(by_chr[c], dtype=np.float64)) for c in chrs]
        q, scale = quantise_weights(np.concatenate(beta, axis=1))
        at = np.cumsum([0] + [b.shape[1] for b in beta])
        return {c: q[:, at[k]:at[k + 1]] for k, c in enumerate(chrs)}, scale

    q, scale = quantised(beta_by_chr)
    out = sums(ctx, pop, q, ind, want=(True, False))[0].astype(np.float64) * scale[:, None]
    if dominance_by_chr is not None:
        qd, scale_d = quantised(dominance_by_chr)
        out = out + sums(ctx, pop, qd, ind, want=(False, True))[1].astype(np.float64) * scale_d[:, None]
    return out
