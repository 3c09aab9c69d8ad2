"""geneevolve_amd/pca.py with its two integer products answered by the host builds (gev_dbg_ind_scores_host, gev_dbg_trait_sums_host)
against numpy.linalg.eigh of the float64 Z Z^T / M.  No device is needed.

The bound is measured here, not fixed: the identical iteration runs with unquantised float64 numpy products, and its own distance from
eigh is what subspace iteration leaves after `ITERS` rounds; the quantised run may exceed that distance by pca.quantisation_allowance,
the first-order cost of 30-bit operands derived in the module's docstring.  Measured on this input (120 + 80 individuals, 2949
polymorphic of 3000 SNPs, spectrum 13.9 : 7.4 : 1.5): relative eigenvalue error float 1.0e-15, quantised 9.8e-12, allowance 5.7e-8; sine
of the largest principal angle float 2.0e-15, quantised 2.5e-10, allowance 1.7e-7."""
import numpy as np
import pytest

from geneevolve_amd import capi, pca

N_A, N_B, N_SNPS, K, ITERS, OVERSAMPLE, BITS = 120, 80, 3000, 2, 20, 8, 30
CHR_AT = [0, 1800, N_SNPS]                                 # two chromosomes: the SNP axis is put together from both


def structured_rows(seed=11):
    """two founder groups (120 + 80 people) whose allele frequencies differ, and inside each a part (50 / 30 people) shifted along a
    second direction, so that two eigenvalues stand clear of the rest; 40 SNPs without allele 1 and 11 without allele 0 among them.
    -> uint8 [400][3000]"""
    rs = np.random.RandomState(seed)
    p0 = rs.uniform(0.15, 0.85, N_SNPS)
    group = [np.clip(p0 + rs.normal(0, 0.12, N_SNPS), 0.02, 0.98) for _ in range(2)]
    shift = rs.normal(0, 0.12, N_SNPS)
    rows = []
    for g, n, n_part in ((0, N_A, 50), (1, N_B, 30)):
        for i in range(n):
            p = np.clip(group[g] + (shift if i < n_part else 0.0), 0.02, 0.98)
            rows.append(rs.random_sample((2, N_SNPS)) < p)
    bits = np.concatenate(rows).astype(np.uint8)
    bits[:, 100:140] = 0
    bits[:, 2500:2511] = 1
    return bits


class HostContext:
    """the calls pca.py makes, answered from rows in host memory: two populations (the founder groups), two chromosomes"""

    def __init__(self, lib, bits01):
        self.lib = lib
        self.rows = {(p, c): capi.pack_rows(bits01[2 * i0:2 * i1, CHR_AT[c]:CHR_AT[c + 1]]) for p, (i0, i1) in enumerate(((0, N_A), (N_A, N_A + N_B))) for c in range(2)}
        self._nsnp = {(p, c): CHR_AT[c + 1] - CHR_AT[c] for p in range(2) for c in range(2)}

    def pop_size(self, pop):
        return (N_A, N_B)[pop]

    def active_chrs(self):
        return [0, 1]

    def snp_genotype_counts(self, pop, chr):
        return self.lib.dbg_snp_counts_host(self.rows[(pop, chr)], self._nsnp[(pop, chr)])

    def host_products(self):
        return (lambda pop, chr, q: self.lib.dbg_ind_scores_host(self.rows[(pop, chr)], self._nsnp[(pop, chr)], q, want=(True, False))[0],
                lambda pop, chr, q: self.lib.dbg_trait_sums_host(self.rows[(pop, chr)], self._nsnp[(pop, chr)], q)[0])


def numpy_products(bits01):
    """the two products in float64 numpy, unquantised"""
    g = (bits01[0::2] + bits01[1::2]).astype(np.float64)
    ind = ((0, N_A), (N_A, N_A + N_B))
    return (lambda pop, chr, w: w @ g[ind[pop][0]:ind[pop][1], CHR_AT[chr]:CHR_AT[chr + 1]].T,
            lambda pop, chr, y: y @ g[ind[pop][0]:ind[pop][1], CHR_AT[chr]:CHR_AT[chr + 1]])


def distances(c, lam, vec):
    """(largest relative eigenvalue error of the leading K, sine of the largest principal angle between the two leading subspaces)"""
    eig = float((np.abs(c.values - lam[:K]) / lam[:K]).max())
    ang = float(np.linalg.norm(c.vectors - vec[:, :K] @ (vec[:, :K].T @ c.vectors), 2))
    return eig, ang


@pytest.fixture(scope="module")
def truth():
    bits = structured_rows()
    g = (bits[0::2] + bits[1::2]).astype(np.float64)
    p = g.mean(axis=0) / 2
    poly = (p > 0) & (p < 1)
    z = (g[:, poly] - 2 * p[poly]) / np.sqrt(2 * p[poly] * (1 - p[poly]))
    lam, vec = np.linalg.eigh(z @ z.T / poly.sum())
    return bits, z, poly, lam[::-1], vec[:, ::-1]


def test_components_against_eigh(gpu_lib, truth):
    bits, z, poly, lam, vec = truth
    n, M = z.shape
    assert M == N_SNPS - 51 and lam[K - 1] > 3 * lam[K], "two eigenvalues stand clear of the rest"
    ctx = HostContext(gpu_lib, bits)
    kw = dict(chrs=None, iters=ITERS, oversample=OVERSAMPLE, seed=3)
    plain = pca.components(ctx, [0, 1], K, bits=None, products=numpy_products(bits), **kw)
    quant = pca.components(ctx, [0, 1], K, bits=BITS, products=ctx.host_products(), **kw)
    allow = pca.quantisation_allowance(lam, n, M, K, K + OVERSAMPLE, BITS)
    d_plain, d_quant = distances(plain, lam, vec), distances(quant, lam, vec)
    print(f"spectrum {lam[:K + 1]}, M {M}")
    for name, a, b, c in zip(("relative eigenvalue error", "sine of the largest principal angle"), d_plain, d_quant, allow):
        print(f"{name}: float64 iteration {a:.3g}, quantised {b:.3g}, allowance {c:.3g}")
    for q in (plain, quant):
        assert q.n_snps == M and q.vectors.shape == (n, K) and np.allclose(q.vectors.T @ q.vectors, np.eye(K), atol=1e-12)
        assert len(q.ritz) == K + OVERSAMPLE and np.array_equal(q.values, q.ritz[:K])
    for a, b, c in zip(d_plain, d_quant, allow):
        assert b <= a + c
    # the monomorphic SNPs are dropped: no loading on them, and the count says so
    mono = np.flatnonzero(~poly)
    whole = np.concatenate([quant.loadings_by_chr[c] for c in range(2)], axis=1)
    assert len(mono) == 51 and not whole[:, mono].any()
    assert (np.abs(whole[:, poly]) > 0).mean() > 0.99


def test_project_gives_the_individuals_their_own_components(gpu_lib, truth):
    """project() of the individuals the components came from: sum_j loadings g - offset is one exact power step Z Z^T u / (M lambda) of
    the returned vector, and that differs from u by the Ritz residual over lambda, which numpy states here from Z itself.  Allowed on
    top: the loadings' quantisation (2 L copies of an error of 2^-31 of the largest loading), the quantised Q behind the loadings
    (lambda_1 / lambda_k sqrt(n) 2^-31, as the module derives for the eigenvalues), and float64 rounding of sums of n + M terms"""
    bits, z, poly, lam, vec = truth
    n, M = z.shape
    ctx = HostContext(gpu_lib, bits)
    c = pca.components(ctx, [0, 1], K, iters=ITERS, oversample=OVERSAMPLE, seed=3, bits=BITS, products=ctx.host_products())
    got = np.concatenate([pca.project(ctx, p, c.loadings_by_chr, c.offset, bits=BITS, products=ctx.host_products()) for p in range(2)])
    step = z @ (z.T @ c.vectors) / (M * c.values)
    residual = np.abs(step - c.vectors)
    whole = np.concatenate([c.loadings_by_chr[k] for k in range(2)], axis=1)
    allow = 2 * N_SNPS * np.abs(whole).max(axis=1) * 2.0 ** -31 + lam[0] / lam[K - 1] * np.sqrt(n) * 2.0 ** -31 + (n + M) * np.finfo(float).eps
    print(f"project - power step {np.abs(got - step).max(axis=0)}, allowance {allow}; power step - vectors {residual.max(axis=0)}")
    assert got.shape == (n, K) and (np.abs(got - step) <= allow[None, :]).all()
    assert (np.abs(got - c.vectors) <= residual + allow[None, :]).all()
    part = pca.project(ctx, 1, c.loadings_by_chr, c.offset, ind=(7, 20), products=ctx.host_products())
    assert np.array_equal(part, got[N_A + 7:N_A + 27])


def test_one_population_one_chromosome(gpu_lib, truth):
    """a population on its own and one chromosome of the two: M and the frequencies are those of the request"""
    bits, z, poly, lam, vec = truth
    ctx = HostContext(gpu_lib, bits)
    c = pca.components(ctx, 0, 1, chrs=[1], iters=6, products=ctx.host_products())
    g = (bits[0:2 * N_A:2, CHR_AT[1]:] + bits[1:2 * N_A:2, CHR_AT[1]:]).astype(np.float64)
    p = g.mean(axis=0) / 2
    ok = (p > 0) & (p < 1)
    zz = (g[:, ok] - 2 * p[ok]) / np.sqrt(2 * p[ok] * (1 - p[ok]))
    top = np.linalg.eigvalsh(zz @ zz.T / ok.sum())[::-1]
    assert c.n_snps == int(ok.sum()) and list(c.loadings_by_chr) == [1] and c.vectors.shape == (N_A, 1)
    # six rounds shrink the tangent of the start's angle (at most about sqrt(n) ~ 10 with 8 spare columns) by (lambda_10 / lambda_1)^(6 + 1/2),
    # a Ritz value errs by the square of that; the 30-bit operands add their allowance
    r = top[9] / top[0]
    allow = pca.quantisation_allowance(top, N_A, c.n_snps, 1, 9, 30)[0]
    print(f"lambda_1 {top[0]:.4g}, lambda_10 / lambda_1 {r:.3g}: error {abs(c.values[0] - top[0]) / top[0]:.3g}, bound {100 * r ** 13 + allow:.3g}")
    assert r < 0.5 and abs(c.values[0] - top[0]) <= (100 * r ** 13 + allow) * top[0]
