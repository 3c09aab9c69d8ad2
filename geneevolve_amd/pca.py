"""Principal components of population structure without a GRM: the leading eigenpairs of Z Z^T / M, Z = (G - 2p) / sqrt(2p(1-p)) over
the M polymorphic SNPs of the chosen populations and chromosomes (individuals x SNPs; p: the pooled frequency of allele 1, from
gev_snp_genotype_counts), by randomised subspace iteration on the device's two integer products: G W (scores.sums, gev_ind_scores) and
G^T Y (assoc.sums, gev_snp_trait_sums).  Nothing larger than individuals x columns and SNPs x columns exists on the host, where the
GRM route (relatedness.pair_counts) holds three matrices of individuals x individuals.

With D = diag(1 / sqrt(2p(1-p))) and c = k + oversample columns
    Z W   = G (D W) - 1 (2p)^T (D W)          the columns of D W quantised to int32 (scores.quantise_weights), the product exact
    Z^T Q = D (G^T Q - 2p (1^T Q))            the columns of Q quantised likewise
the rank-one mean terms are formed in float64 from the QUANTISED columns, so each product is the exact product of Z with a matrix
whose entries are off by at most 2^-(bits+1) of their column's largest.  The iteration is Y = Z Omega, Q = qr(Y), then `iters` times
B = qr(Z^T Q), Q = qr(Z B), and at the end B = Z^T Q and the c x c eigenproblem of B^T B / M; the vectors are Q V.

What quantisation costs, to first order (quantisation_allowance).  Columns of Q and of qr(Z^T Q) have norm 1, so an entry is off by at
most 2^-(bits+1) and a whole operand of r rows and c columns by sqrt(r c) 2^-(bits+1) in norm; Z turns that into at most sigma_1 =
sqrt(M lambda_1) times as much.
  eigenvalues: a Ritz value moves with the square of the subspace's error, so to first order only the last product counts:
      lambda_i = |B v_i|^2 / M,  |dB| <= sigma_1 sqrt(n c) 2^-(bits+1)   =>   |d lambda| / lambda_i <= sqrt(n c) 2^-bits sqrt(lambda_1 / lambda_i)
  subspace: a half step's error enters the leading k-subspace relative to sigma_k, the next half steps shrink it by lambda_(k+1) /
      lambda_k per round (a geometric series), and both kinds of half step contribute:
      sin(angle) <= sqrt(c) 2^-(bits+1) sqrt(lambda_1 / lambda_k) (sqrt(M) + sqrt(n)) / (1 - lambda_(k+1) / lambda_k)
At bits = 30, n = 200, M = 2949, c = 10 and the spectrum 13.9 : 7.4 : 1.5 of tests/test_pca_cpu.py these are 5.7e-8 and 1.7e-7; measured
there: 9.8e-12 and 2.5e-10 (the bound takes every rounding error at its largest and all of them aligned; the float64 iteration itself
stands 1e-15 and 2e-15 from eigh after 20 rounds)."""
from collections import namedtuple

import numpy as np

from . import assoc, scores
from ._ranges import chrs as _chrs

Components = namedtuple("Components", "values vectors loadings_by_chr offset n_snps ritz")
Components.__doc__ = """values: float64 [k], the leading eigenvalues of Z Z^T / M, descending; vectors: float64 [n][k], orthonormal columns, the
individuals of the populations in the order given; loadings_by_chr: chr -> float64 [k][L] and offset: float64 [k], so that component s of
ANY individual with genotypes g is sum_j loadings[s][j] g_j - offset[s] (project); zero at the SNPs left out; n_snps: M, the polymorphic
SNPs; ritz: float64 [k + oversample], all the Ritz values of the last subspace (values and what lies behind them)"""


def quantisation_allowance(spectrum, n, M, k, cols, bits):
    """(relative eigenvalue error, sine of the largest principal angle) that quantising the operands to `bits` bits may add to the
    leading k eigenpairs, to first order (module docstring); spectrum: at least the k + 1 largest eigenvalues, descending"""
    lam = np.asarray(spectrum, dtype=np.float64)
    eig = np.sqrt(n * cols) * 2.0 ** -bits * np.sqrt(lam[0] / lam[k - 1])
    ang = np.sqrt(cols) * 2.0 ** -(bits + 1) * np.sqrt(lam[0] / lam[k - 1]) * (np.sqrt(M) + np.sqrt(n)) / (1.0 - lam[k] / lam[k - 1])
    return float(eig), float(ang)


def _device_products(ctx):
    """the two integer products from the device: (pop, chr, q int32 [cols][L]) -> G q^T int64 [cols][n], (pop, chr, q int32 [cols][n]) ->
    G^T q^T int64 [cols][L]"""
    return (lambda pop, chr, q: scores.sums(ctx, pop, {chr: q}, want=(True, False))[0],
            lambda pop, chr, q: assoc.sums(ctx, pop, chr, q).gsum)


def _quantised(a, bits):
    """columns given as rows [cols][m] -> (q, scale [cols]): what goes into the product and the factor back to what it stands for"""
    if bits is None:
        return a, np.ones(a.shape[0])
    return scores.quantise_weights(a, bits)


class _Z:
    """Z of the chosen populations and chromosomes as two products; SNP axis: the chromosomes one behind another, monomorphic SNPs kept
    with weight 0; individual axis: the populations one behind another"""

    def __init__(self, ctx, pops, chrs, bits, products):
        self.pops, self.chrs, self.bits = pops, chrs, bits
        self.gw, self.gty = products if products is not None else _device_products(ctx)
        n_of = [ctx.pop_size(p) for p in pops]
        L_of = [ctx._nsnp[(pops[0], c)] for c in chrs]
        assert all(ctx._nsnp[(p, c)] == L for p in pops for c, L in zip(chrs, L_of)), "the populations share their SNPs"
        self.n = sum(n_of)
        alt = np.zeros(sum(L_of), dtype=np.int64)                                                  # copies of allele 1 per SNP
        self.snp_at, self.ind_at = np.cumsum([0] + L_of), np.cumsum([0] + n_of)
        for ic, c in enumerate(chrs):
            for p in pops:
                het, hom = ctx.snp_genotype_counts(p, c)
                alt[self.snp_at[ic]:self.snp_at[ic + 1]] += het.astype(np.int64) + 2 * hom.astype(np.int64)
        self.p = alt / (2.0 * self.n)
        poly = (alt > 0) & (alt < 2 * self.n)
        self.M = int(poly.sum())
        self.d = np.zeros(len(alt))
        self.d[poly] = 1.0 / np.sqrt(2.0 * self.p[poly] * (1.0 - self.p[poly]))

    def z_times(self, W):
        """Z W, W: [L_total][cols] -> [n][cols]"""
        q, scale = _quantised((self.d[:, None] * W).T, self.bits)
        g = np.concatenate([sum(self.gw(pop, chr, np.ascontiguousarray(q[:, self.snp_at[ic]:self.snp_at[ic + 1]])) for ic, chr in enumerate(self.chrs))
                            for pop in self.pops], axis=1)                                         # G q^T: [cols][n], exact for integer q
        return ((g - (q @ (2.0 * self.p))[:, None]) * scale[:, None]).T

    def zt_times(self, Q):
        """Z^T Q, Q: [n][cols] -> [L_total][cols]"""
        q, scale = _quantised(Q.T, self.bits)
        g = np.concatenate([sum(self.gty(pop, chr, np.ascontiguousarray(q[:, self.ind_at[ip]:self.ind_at[ip + 1]])) for ip, pop in enumerate(self.pops))
                            for chr in self.chrs], axis=1)                                         # G^T q^T: [cols][L_total]
        return ((g - q.sum(axis=1, dtype=np.float64)[:, None] * (2.0 * self.p)[None, :]) * (scale[:, None] * self.d[None, :])).T


def components(ctx, pops, k, chrs=None, iters=4, oversample=8, seed=1, bits=30, products=None):
    """the leading k eigenpairs of Z Z^T / M over the current generations of `pops` (one population index or several, which share their
    SNPs) and the chromosomes `chrs` (None: the active ones) -> Components.  iters: rounds of the subspace iteration after the first
    range finding (the error falls by lambda_(k+oversample+1) / lambda_k per round); bits: of the quantised operands (None with
    caller-supplied float products: no quantisation).  products: (gw, gty) as _device_products gives them, in place of the device: the
    host builds (gev_dbg_ind_scores_host, gev_dbg_trait_sums_host) or numpy"""
    pops = [int(pops)] if np.ndim(pops) == 0 else [int(p) for p in pops]
    Z = _Z(ctx, pops, _chrs(ctx, chrs), bits, products)
    c = min(k + oversample, Z.n, Z.M)
    assert 1 <= k <= c, "more components than individuals or polymorphic SNPs"
    omega = np.random.RandomState(seed).standard_normal((len(Z.p), c))
    Q = np.linalg.qr(Z.z_times(omega))[0]
    for _ in range(iters):
        B = np.linalg.qr(Z.zt_times(Q))[0]
        Q = np.linalg.qr(Z.z_times(B))[0]
    B = Z.zt_times(Q)
    lam, V = np.linalg.eigh(B.T @ B / Z.M)
    order = np.argsort(lam)[::-1]
    lam, V = lam[order], V[:, order]
    U = Q @ V[:, :k]
    load = (B @ V[:, :k]) / (Z.M * lam[:k])[None, :] * Z.d[:, None]                               # [L_total][k]: D Z^T u / (M lambda)
    loadings = {chr: np.ascontiguousarray(load[Z.snp_at[ic]:Z.snp_at[ic + 1]].T) for ic, chr in enumerate(Z.chrs)}
    return Components(lam[:k], U, loadings, load.T @ (2.0 * Z.p), Z.M, lam)


def project(ctx, pop, loadings_by_chr, offset, ind=None, bits=30, products=None):
    """the components of the individuals `ind` of `pop` (None: everybody, or (begin, n)) -- of the individuals the components were
    computed from, or of new ones typed at the same SNPs -> float64 [n_ind][k]: sum_j loadings[s][j] g_ij - offset[s], the loadings
    quantised with one scale per component over all chromosomes.  products: (gw, gty) in place of the device, gw over everybody of pop"""
    chrs = sorted(loadings_by_chr)
    load = [np.atleast_2d(np.asarray(loadings_by_chr[c], dtype=np.float64)) for c in chrs]
    at = np.cumsum([0] + [a.shape[1] for a in load])
    q, scale = scores.quantise_weights(np.concatenate(load, axis=1), bits)
    by_chr = {c: np.ascontiguousarray(q[:, at[i]:at[i + 1]]) for i, c in enumerate(chrs)}
    if products is None:
        g = scores.sums(ctx, pop, by_chr, ind, want=(True, False))[0]
    else:
        g = sum(products[0](pop, c, by_chr[c]) for c in chrs)
        if ind is not None:
            g = g[:, ind[0]:ind[0] + ind[1]]
    return (g.astype(np.float64) * scale[:, None] - np.asarray(offset, dtype=np.float64)[:, None]).T
