"""The digit-column product that the trait sums and the scores share (geneevolve_amd/csrc/gev_digitprod.h), through the host builds of both
sides on one population: gev_dbg_ind_scores_host (G W) and gev_dbg_trait_sums_host (G^T Y) against plain numpy, the one refusal check under
both in each side's words, and assoc.quantise, which is scores.quantise_weights after centring, against its formula written out.  Every
comparison is exact.  No device is needed."""
import numpy as np
import pytest

from geneevolve_amd import assoc, capi
from tests.ind_scores_inputs import L, N_PEOPLE, genotypes, numpy_scores, population_rows, random_weights
from tests.trait_sums_inputs import numpy_trait_sums, random_quanta

# (SNPs, individuals, columns): everything with more columns than four column groups hold evenly, then a sub-range of each side
CASES = [((0, L), (0, N_PEOPLE), 17), ((63, 130), (5, 129), 1), ((56, 15), (100, 1), 1), ((4033, 127), (133, 17), 5)]


@pytest.fixture(scope="module")
def population():
    bits = population_rows()
    return bits, genotypes(bits), capi.pack_rows(bits)


@pytest.mark.parametrize("snps,ind,n_cols", CASES, ids=lambda v: str(v))
def test_both_host_products_equal_numpy(gpu_lib, population, snps, ind, n_cols):
    bits, geno, rows = population
    (s0, ns), (i0, ni) = snps, ind
    rs = np.random.RandomState(n_cols + ns)
    w = random_weights(rs, n_cols, ns)
    for got, want in zip(gpu_lib.dbg_ind_scores_host(rows, L, w, s0, ns, i0, ni), numpy_scores(geno, s0, ns, i0, ni, w)):
        assert got.dtype == np.int64 and np.array_equal(got, want), f"scores: differ at {np.argwhere(got != want)[:5].tolist()}"
    q = random_quanta(rs, n_cols, ni)
    for got, want in zip(gpu_lib.dbg_trait_sums_host(rows, L, q, s0, ns, i0, ni), numpy_trait_sums(bits, s0, ns, i0, ni, q)):
        assert got.shape == want.shape and np.array_equal(got, want), f"trait sums: differ at {np.argwhere(got != want)[:5].tolist()}"


def test_one_check_refuses_in_each_sides_words(gpu_lib, population):
    """the texts of the three refusals that the two calls share, as they were when each call had a check of its own"""
    bits, geno, rows = population
    ts, sc = gpu_lib._f("dbg_trait_sums_host"), gpu_lib._f("dbg_ind_scores_host")
    out = np.zeros((2, 5), dtype=np.int64)
    big = (1 << 22) + 1
    assert ts(None, 0, big, 10, 0, 1, 0, big, None, 1, None, None, None, None) == -5
    assert gpu_lib.last_error() == f"dbg_trait_sums_host: {big} individuals in one call, at most {1 << 22} (a digit's sum is an int32)"
    assert sc(None, 0, 10, big, 0, big, 0, 1, None, 1, None, None) == -5
    assert gpu_lib.last_error() == f"dbg_ind_scores_host: {big} SNPs in one call, at most {1 << 22} (a digit's sum is an int32)"
    assert ts(rows, rows.shape[1], N_PEOPLE, L, 0, 5, 0, 5, None, 2, out, None, None, None) == -1
    assert gpu_lib.last_error() == "dbg_trait_sums_host: null trait array (2 traits of 5 quanta each)"
    assert sc(rows, rows.shape[1], N_PEOPLE, L, 0, 5, 0, 5, None, 2, out, None) == -1
    assert gpu_lib.last_error() == "dbg_ind_scores_host: null weight array (2 columns of 5 weights each)"
    bad = np.zeros((2, 5), dtype=np.int32); bad[1, 3] = -(1 << 30) - 1
    assert ts(rows, rows.shape[1], N_PEOPLE, L, 0, 5, 0, 5, bad, 2, out, None, None, None) == -1
    assert gpu_lib.last_error() == f"dbg_trait_sums_host: quantum {bad[1, 3]} of trait 1, individual 3 beyond +-2^30"
    assert sc(rows, rows.shape[1], N_PEOPLE, L, 0, 5, 0, 5, bad, 2, out, None) == -1
    assert gpu_lib.last_error() == f"dbg_ind_scores_host: weight {bad[1, 3]} of column 1, SNP 3 beyond +-2^30"


def quantise_written_out(y, bits=30):
    """assoc.quantise as it stood before it called scores.quantise_weights"""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    if y.shape[1] == 0:
        return np.zeros(y.shape, dtype=np.int32), np.ones(y.shape[0]), np.zeros(y.shape[0])
    mean = y.mean(axis=1)
    dev = y - mean[:, None]
    top = np.abs(dev).max(axis=1)
    scale = np.where(top > 0, top / float(1 << bits), 1.0)
    q = np.clip(np.rint(dev / scale[:, None]), -(1 << bits), 1 << bits).astype(np.int32)
    return q, scale, mean


@pytest.mark.parametrize("y", [np.random.RandomState(1).normal(3.0, 2.0, (3, 50)), np.full((1, 20), 2.5), np.zeros((2, 0))],
                         ids=["random 3 x 50", "a constant trait", "no individuals"])
def test_quantise_is_its_formula_bit_for_bit(y):
    for bits in (30, 12):
        got, want = assoc.quantise(y, bits), quantise_written_out(y, bits)
        for name, g, x in zip(("q", "scale", "mean"), got, want):
            assert g.dtype == x.dtype and g.shape == x.shape and np.array_equal(g, x), (name, bits)
