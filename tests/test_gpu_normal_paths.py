"""The normal streams and the mean / variance sums are one piece of device code with three callers (csrc/gev_normal.h:
gev_scale_ad_compute_gef, gev_generation_phenotypes, gev_compute_selection).  These tests pin what the callers share, bit for bit, at
the smallest sizes where the shared code takes another path.  Nothing here has a tolerance: both sides of every comparison run the
same kernels on the same numbers."""
import math

import numpy as np
import pytest

from geneevolve_amd.host import SyntheticConfig
from tests.helpers import bits_equal

pytestmark = pytest.mark.gpu


def population(gpu_lib, n, nphen, rng_seed):
    """one context, one population of n with pedigree ids on the device and raw A/D set from the host (nothing depends on genotypes)"""
    cfg = SyntheticConfig(max(n, 2), 256, chrom_bp=2_000_000, map_step=10_000, n_cv=16, nphen=nphen, seed=3)
    ctx = gpu_lib.create(1, 1, nphen)
    ctx.set_track_pedigree(True)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 5)
    for p in range(nphen):
        ctx.synth_cv_founders(0, p, 0, 2 * n, 13 + p)
    ctx.init_gen0(0, n, 780)
    rng = np.random.default_rng(rng_seed)
    ctx.set_ad(0, rng.standard_normal((n, nphen)), rng.standard_normal((n, nphen)))
    return ctx


# (n/2 + 1) / 0.7 + 4096 candidate pairs are exactly three blocks of 2048 at n = 2866 (even) and 2867 (odd: the last pair half used),
# so the last block is full; 1 to 3 use half a pair and have var(e) = 0 or nearly; 100 003 is many blocks
@pytest.mark.parametrize("n", [1, 2, 3, 2866, 2867, 100_003])
def test_both_entry_points_draw_and_scale_alike(gpu_lib, n):
    """gev_generation_phenotypes at generation 0 (two phenotypes, ve, vf > 0, vc = 0), then gev_scale_ad_compute_gef on a twin context
    with the seeds the step reports: E, F and P bit for bit"""
    if n in (2866, 2867):
        assert int((n // 2 + 1) / 0.7) + 4096 == 3 * 2048
    schemes = [(0.5, 0.2, 0.0, 0.4, 0.3, 1.0), (0.6, 0.0, 0.0, 0.2, 0.1, 1.0)]           # va, vd, vc, ve, vf, beta
    a, b = population(gpu_lib, n, 2, n), population(gpu_lib, n, 2, n)
    a.generation_phenotypes(0, 0, 4242, schemes)
    seeds = a.phenotypes_result(0)["seeds"]
    assert len(seeds) == 2
    for p, (va, vd, _, ve, vf, beta) in enumerate(schemes):
        s2_a, s2_d = a.get_ad_gen0(0, p)
        want = a.download_phenotypes(0, p)
        got = b.scale_ad_compute_gef(0, p, 0, int(seeds[p]), va, vd, ve, vf, beta, s2_a, s2_d)
        for name in ("e_noise", "parental_effect", "phen", "additive", "dominance", "bv"):
            assert bits_equal(got[name], want[name]), f"n = {n}, phenotype {p}: {name} differs between the two entry points"
        if n == 1:
            assert got["e_noise"][0] == 0.0, "var of one value is 0"
    a.close(); b.close()


@pytest.mark.parametrize("n", [2867, 100_003])
def test_gef_runs_again_when_its_streams_are_short(gpu_lib, n):
    """with the test knob the first attempt has n / 4 + 16 candidate pairs: the call runs again and returns the same bits; the rerun
    counter moves; the phenotypes it keeps are accepted by gev_compute_selection"""
    out = []
    for short in (False, True):
        ctx = population(gpu_lib, n, 1, n)
        before = ctx.dbg_phenotype_knobs(short)
        out.append(ctx.scale_ad_compute_gef(0, 0, 0, 777, 0.5, 0.2, 0.4, 0.3, 1.0, 1.7, 0.3))
        reruns = ctx.dbg_phenotype_knobs(False) - before
        assert reruns == (1 if short else 0), f"n = {n}, short = {short}: {reruns} reruns"
        mv = ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0], want=("mating_value",))["mating_value"]
        assert bits_equal(mv, out[-1]["phen"]), "the kept phenotype column is the returned one"
        ctx.close()
    for name in out[0]:
        assert bits_equal(out[0][name], out[1][name]), f"n = {n}: {name} differs after the rerun"


def tree_mean_var(x):
    """CommFunc::mean / CommFunc::var as k_ph_var_partial / k_ph_var_final sum them, in numpy: min(ceil(n/256), 256) blocks of 256
    threads, each thread its grid-stride elements in order, a halving tree per block, the block sums through the same tree"""
    n = len(x)
    nb = min(math.ceil(n / 256), 256)

    def total(v):
        t = nb * 256
        padded = np.zeros(math.ceil(n / t) * t)
        padded[:n] = v
        acc = np.zeros(t)
        for row in padded.reshape(-1, t):                    # (a thread past the end adds nothing: + 0.0 leaves the sum's bits)
            acc = acc + row
        s = acc.reshape(nb, 256).copy()
        w = 128
        while w:
            s[:, :w] += s[:, w:2 * w]; w //= 2
        f = np.zeros(256); f[:nb] = s[:, 0]
        w = 128
        while w:
            f[:w] += f[w:2 * w]; w //= 2
        return f[0]

    mean = total(x) / n
    if n <= 1:
        return mean, 0.0
    dev = x - mean
    return mean, total(dev * dev) / (n - 1)


# where the sum gets a second thread's worth (2), a second block (257) and a second element per thread (65 537), and their neighbours
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65_536, 65_537])
def test_generation0_selection_statistics_are_the_shared_sum(gpu_lib, n):
    """one phenotype, lambda = 1, no shift: sv is the P plane.  gev_get_selection_gen0 gives, bit for bit, the variance that
    gev_phenotypes_result reports for P (the ABI hands out the variances of the component statistics, not their means) and the
    {mean, var} of the summation order written out in numpy"""
    ctx = population(gpu_lib, n, 1, n)
    ctx.generation_phenotypes(0, 0, 99, [(0.5, 0.2, 0.0, 0.4, 0.3, 1.0)])
    var_p = ctx.phenotypes_result(0)["var"][0][6]
    sv = ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0], want=("mating_value",))["mating_value"]
    assert bits_equal(sv, ctx.download_phenotypes(0, 0)["phen"])
    mean, var = ctx.get_selection_gen0(0)
    want_mean, want_var = tree_mean_var(sv)
    assert bits_equal([var], [var_p]), f"n = {n}: generation-0 variance {var!r}, the P component's {var_p!r}"
    assert bits_equal([mean, var], [want_mean, want_var]), f"n = {n}: {(mean, var)!r}, summation order in numpy {(want_mean, want_var)!r}"
    if n == 1:
        assert var == 0.0
    ctx.close()
