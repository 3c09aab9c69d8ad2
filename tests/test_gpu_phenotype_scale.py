"""Device phenotype scaling (gev_scale_ad_compute_gef: the parallel polar-method normal stream, the two-pass variance of e, the
scaling branches) and the selection values computed from the phenotypes it keeps (gev_compute_selection), pinned to the reference's
arithmetic at the benchmark's population size and beyond: Simulation::ras_scale_AD_compute_GEF (reference src/Simulation.cpp:3075-3206),
ras_compute_mating_value_selection_value (:3300-3342) and ras_selection_func (:3386-3428).

Twin contexts (product and CPU oracle) hold the same sexes and the same raw A/D, injected with set_ad, so nothing depends on genotypes.
Outputs that are one IEEE operation of identical inputs on both sides are compared bit for bit; the others against an exact or
correctly rounded value, within bounds derived below.  "ulp" is the distance in doubles (helpers.ulp_distance), eps = 2**-52.

Measured on an MI355X (the max over every value these tests check; `pytest -s` prints the "measured" lines), and the bounds set from
them: at most twice the measurement, rounded up to a power of two, and no device bound looser than 1e-13 relative except the two
named below, where the formula itself scales a libm error.
- Normal stream, device log / sqrt against glibc's in libstdc++'s polar method: max 4 ulps (n = 1 000 001; 3 ulps up to 100 000,
  0 for n <= 3).  Bound STREAM_ULP = 8 ulps.
- e_noise against the exact value (sec. b): the device max 3.5 eps relative (n = 1 000 001; 2.0 at 65 536), bound derived from its
  summation order, STREAM_ULP + ceil(n / 65536) + 16 + 4 eps (44 eps = 1e-14 at 10**6).  The oracle's sequential sum max 73 eps at
  10**6, bound n + 4 eps (worst case).
- Sec. c, outputs through the stream or the variance, device against oracle: max 50.6 eps (relative for e_noise and the
  generation-0 parental effect, of the magnitudes of its terms for phen), most of it the oracle's sequential sum.  Bound
  GEF_EPS = 128 eps (2.8e-14).
- Generation-0 mean and variance of the selection value at 10**6 (sec. e): 0 eps from the exact values (they round to the same
  double); bound (ceil(n / 65536) + 18) eps of the mean magnitude, (ceil(n / 65536) + 20) eps of the variance.
- Selection functions at the device's own z against the C formula with correctly rounded libm (sec. e): default and logit max
  2 ulps, bound 4 ulps.  probit max 2**-53 absolute, bound 2**-52 absolute: the formula's 1 + erf cancels in the lower tail, so the
  error there is erf's ulp near 1, not an ulp of the result (named exception).  stab max 2.99 ulps per unit of max(1, |exp's
  argument|), bound 4 per unit: an ulp of pow(x, 2) moves exp's argument by that much, and exp multiplies it by the argument, up to
  ~700 (named exception: stated as that product).
"""
import math

import numpy as np
import pytest

from geneevolve_amd.host import SyntheticConfig, ras_selection_func
from oracle import oracle_api
from tests.helpers import GEF_OUTPUTS, c_selection_formula, gef_exact_outputs, ulp_distance

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
STREAM_ULP = 8          # device normal stream against libstdc++'s (glibc log / sqrt)
GEF_EPS = 128           # sec. c: non-exact GEF outputs, device against oracle, in eps of the magnitudes summed into phen
S2_A, S2_D = 1.7, 0.3   # _var_a_gen0 / _var_d_gen0 handed to every call


def record(what, value):
    """the measured distances quoted in the module docstring come from these lines (pytest -s)"""
    print(f"measured {what}: {value}")


def raw_ad(n, rng):
    """[n][3] raw additive and dominance values: N(0,1), a large common offset 1e6 + N(0,1), a constant column"""
    a = np.stack([rng.standard_normal(n), 1e6 + rng.standard_normal(n), np.full(n, 0.625)], axis=1)
    d = np.stack([rng.standard_normal(n), -3e5 + rng.standard_normal(n), np.full(n, -0.375)], axis=1)
    return a, d


def twins(gpu_lib, oracle_lib, n, seed=3, a=None, d=None):
    """one GPU and one oracle context, one population of n with three phenotypes and equal sexes, the same raw A/D set in both"""
    cfg = SyntheticConfig(max(n, 2), 256, chrom_bp=2_000_000, map_step=10_000, n_cv=16, nphen=3, seed=seed)
    g, o = gpu_lib.create(1, 1, 3), oracle_lib.create(1, 1, 3)
    cfg.apply_static(g); cfg.apply_static(o)
    g.synth_founders(0, 0, 2 * n, seed + 2)
    for p in range(3):
        g.synth_cv_founders(0, p, 0, 2 * n, seed + 10 + p)
    assert np.array_equal(g.init_gen0(0, n, 777 + seed), o.init_gen0(0, n, 777 + seed)), "generation-0 sexes differ"
    if a is None:
        a, d = raw_ad(n, np.random.default_rng(n + seed))
    g.set_ad(0, a, d); o.set_ad(0, a, d)
    return g, o


def exact_mean_var(x):
    """CommFunc::mean / CommFunc::var (n - 1) of x, computed to (nearly) the exact real values: fsum is an exactly rounded sum, and
    (x - mu)^2 is summed from its error-free parts (TwoSum for x - mu, Veltkamp / Dekker for the square)"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    mu = math.fsum(x.tolist()) / n
    if n <= 1:
        return mu, 0.0
    dd = x - mu
    bb = dd - x
    err = (x - (dd - bb)) + (-mu - bb)                  # x - mu == dd + err exactly
    sp = dd * 134217729.0                               # 2**27 + 1
    hi = sp - (sp - dd); lo = dd - hi
    sq_hi = dd * dd
    sq_lo = ((hi * hi - sq_hi) + 2 * hi * lo) + lo * lo  # dd * dd == sq_hi + sq_lo exactly
    ss = math.fsum(np.concatenate([sq_hi, sq_lo, 2 * dd * err, err * err]).tolist())
    return mu, ss / (n - 1)


def gef(ctx, phen, gen, seed, va, vd, ve, vf, beta=1.0, cs=None, ff=None, fm=None):
    return ctx.scale_ad_compute_gef(0, phen, gen, seed, va, vd, ve, vf, beta, S2_A, S2_D, common_sibling=cs, f_father=ff, f_mother=fm)


def first_bit_difference(a, b):
    bad = np.flatnonzero(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) != np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))
    return None if len(bad) == 0 else (int(bad[0]), len(bad), float(np.asarray(a)[bad[0]]), float(np.asarray(b)[bad[0]]))


# ---- a. the polar-method stream itself -----------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 4095, 65_535, 65_536, 65_537, 100_000, 1_000_001]
SEEDS = [1, 999_999, 2_147_483_646, 2_147_483_647, 4_294_967_295]


@pytest.mark.parametrize("n", SIZES)
def test_generation0_parental_stream_is_libstdcxx_normal_distribution(gpu_lib, oracle_lib, n):
    """generation 0, vf > 0: parental_effect is the raw N(0, sqrt(vf)) stream of generator_f(seed + 1) (:3095-3114), unscaled.
    n = 65 536 is where k_ph_var_partial starts to stride; 1 000 001 is odd (the last pair half used) and its ~718k candidates are
    351 blocks: k_nrm_emit's threads sum more than one block count each.  Seeds: seed + 1 = 2**31 - 1 (engine state 1), seed = 2**31 - 1, and seed + 1
    wrapping to 0 in unsigned arithmetic, as in the reference.  A misaligned pair after a rejection moves values by O(1)."""
    g, o = twins(gpu_lib, oracle_lib, n)
    vf = 0.3
    worst = []
    for seed in SEEDS:
        want = oracle_api.kat_normal(oracle_lib, (seed + 1) & 0xFFFFFFFF, math.sqrt(vf), n)
        ora = gef(o, 0, 0, seed, 0.5, 0.2, 0.4, vf)["parental_effect"]
        assert first_bit_difference(ora, want) is None, "the oracle's stream is libstdc++'s"
        got = gef(g, 0, 0, seed, 0.5, 0.2, 0.4, vf)["parental_effect"]
        d = ulp_distance(got, want)
        i = int(np.argmax(d))
        worst.append((float(d[i]), seed, i, float(got[i]), float(want[i])))
    record(f"stream ulp n={n} (ulps, seed, index, device, libstdc++)", max(worst))
    for d, seed, i, a, b in worst:
        assert d <= STREAM_ULP, f"seed {seed}, n {n}: parental stream {d} ulps from libstdc++'s at index {i} ({a!r} vs {b!r})"
    g.close(); o.close()


# ---- b. e_noise against the exact variance -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4095, 65_536, 65_537, 1_000_001])
def test_e_noise_is_within_the_tree_sum_bound_of_the_exact_value(gpu_lib, oracle_lib, n):
    """e_noise = e / sqrt(var(e) / ve) (:3167-3169, :3178), e = N(0,1) of generator_e(seed).  The expected value uses the exact
    variance of libstdc++'s stream; the device's two passes sum as a tree (ceil(n/65536) terms per thread, then 8 + 8 levels), the
    oracle sequentially.  ve = 0 gives exactly 0, and so does n = 1 (CommFunc::var of one value is 0)."""
    g, o = twins(gpu_lib, oracle_lib, n)
    ve = 0.4
    worst_d = worst_o = 0.0
    for seed in (12345, 2_147_483_646):
        e = oracle_api.kat_normal(oracle_lib, seed, 1.0, n)
        _, var = exact_mean_var(e)
        got = gef(g, 1, 0, seed, 0.5, 0.2, ve, 0.0)["e_noise"]
        ora = gef(o, 1, 0, seed, 0.5, 0.2, ve, 0.0)["e_noise"]
        if n == 1:
            assert got[0] == 0.0 and ora[0] == 0.0, "var of one value is 0: e_noise 0"
            continue
        scale = math.sqrt(var / ve)
        want = e / scale                               # within an ulp of the exact e / sqrt(var / ve)
        rel = lambda x: np.max(np.abs(x - want) / np.maximum(np.abs(want), 1e-300)) / EPS
        bd = STREAM_ULP + math.ceil(n / 65536) + 16 + 4
        bo = n + 4
        assert rel(got) <= bd, f"device e_noise {rel(got):.1f} eps from the exact value (bound {bd}), seed {seed}"
        assert rel(ora) <= bo, f"oracle e_noise {rel(ora):.1f} eps from the exact value (bound {bo}), seed {seed}"
        worst_d, worst_o = max(worst_d, rel(got)), max(worst_o, rel(ora))
        for ctx in (g, o):
            z = gef(ctx, 1, 0, seed, 0.5, 0.2, 0.0, 0.0)["e_noise"]
            assert first_bit_difference(z, np.zeros(n)) is None, "ve = 0: e_noise exactly 0"
    record(f"e_noise eps n={n} device / oracle", (worst_d, worst_o))
    g.close(); o.close()


# ---- c. every branch of GEF against the oracle ---------------------------------------------------------------------------------
N_C = 100_003
VA, VD, VE, VF = (0.5, 0.0, -1.0), (0.2, 0.0, -1.0), (0.4, 0.0), (0.3, 0.0)


def gef_cases():
    """va x vd x ve x vf x generation in full (72 calls); parents (both / father only / none), common sibling effect (given / None)
    and phenotype (0, 1, 2) staggered across them so that every value of every factor meets every generation and variance"""
    k = 0
    for va in VA:
        for vd in VD:
            for ve in VE:
                for vf in VF:
                    for gen in (0, 2):
                        yield va, vd, ve, vf, gen, ("both", "father", "none")[k % 3], (k // 3) % 2 == 0, (k + k // 6) % 3
                        k += 1


def test_every_gef_branch_matches_the_oracle(gpu_lib, oracle_lib):
    """additive, dominance, bv and generation > 0's parental effect bit for bit; phen too when ve = 0 and (vf = 0 or generation > 0);
    e_noise and generation 0's parental stream within GEF_EPS eps of themselves, phen otherwise within GEF_EPS eps of the magnitudes
    summed into it"""
    n = N_C
    g, o = twins(gpu_lib, oracle_lib, n)
    rng = np.random.default_rng(17)
    cs_v, ff_v, fm_v = rng.standard_normal(n) * 0.3, rng.standard_normal(n), rng.standard_normal(n)
    worst = 0.0
    seen = set()
    for i, (va, vd, ve, vf, gen, parents, with_cs, ph) in enumerate(gef_cases()):
        seen.add((parents, with_cs, ph))
        ff = ff_v if parents in ("both", "father") else None
        fm = fm_v if parents == "both" else None
        cs = cs_v if with_cs else None
        seed = 1000 + 7919 * i
        got, want = (gef(ctx, ph, gen, seed, va, vd, ve, vf, beta=0.7, cs=cs, ff=ff, fm=fm) for ctx in (g, o))
        label = f"va={va} vd={vd} ve={ve} vf={vf} gen={gen} parents={parents} cs={with_cs} phen={ph}"
        exact = gef_exact_outputs(gen, ve, vf)
        mag = sum(np.abs(want[k]) for k in ("additive", "dominance", "e_noise", "parental_effect")) + (np.abs(cs) if cs is not None else 0.0)
        for nm in GEF_OUTPUTS:
            if nm in exact:
                diff = first_bit_difference(got[nm], want[nm])
                assert diff is None, f"{label}: {nm} not bit-identical: first at index {diff[0]} ({diff[1]} values; {diff[2]!r} vs {diff[3]!r})"
            else:
                scale = mag if nm == "phen" else np.abs(want[nm])
                err = np.max(np.abs(got[nm] - want[nm]) / np.maximum(scale, 1e-300)) / EPS
                assert err <= GEF_EPS, f"{label}: {nm} {err:.1f} eps from the oracle (bound {GEF_EPS})"
                worst = max(worst, float(err))
    assert {p for p, _, _ in seen} == {"both", "father", "none"} and {c for _, c, _ in seen} == {True, False} and {h for _, _, h in seen} == {0, 1, 2}
    record("GEF eps device vs oracle n=100003", worst)
    g.close(); o.close()


# ---- d. the phenotypes the library keeps for selection --------------------------------------------------------------------------
N_BIG = 1_000_001


def test_kept_phenotypes_are_the_returned_ones(gpu_lib, oracle_lib):
    """after GEF of phenotypes 0, 1, 2, compute_selection with omega = e_k gives phenotype k's phen output bit for bit
    (0 + 1.0 x + 0 y + ... is x): a wrong stride or column in k_gef_apply's write of the kept phenotypes shows here"""
    n = N_BIG
    g, o = twins(gpu_lib, oracle_lib, n)
    o.close()
    phen = [gef(g, p, 0, 4242 + p, (0.5, 0.6, -1.0)[p], (0.2, 0.0, 0.1)[p], (0.4, 0.0, 0.3)[p], (0.0, 0.3, 0.0)[p])["phen"] for p in range(3)]
    for k in range(3):
        omega = [1.0 if p == k else 0.0 for p in range(3)]
        mv = g.compute_selection(0, 0, "none", 0, 0, omega, [1.0, 1.0, 1.0], want=("mating_value",))["mating_value"]
        diff = first_bit_difference(mv, phen[k])
        assert diff is None, f"mating value with omega = e_{k} is not phenotype {k}: first at index {diff[0]} ({diff[1]} values; {diff[2]!r} vs {diff[3]!r})"
    g.close()


# ---- e. selection values at scale on identical inputs ---------------------------------------------------------------------------
FUNCS_E = [("", 0.0, 0.0), ("logit", 1.0, 1.0), ("probit", -0.3, 0.8), ("stab", 0.2, 1.3), ("stab", 0.1, 0.05), ("thr", 0.4, None), ("none", 0.0, 0.0)]


def func_error(kind, p1, p2, got, want, z):
    """the distance of a selection-function value from the C formula, in the unit its bound is stated in (module docstring)"""
    if kind == "probit":
        return np.abs(got - want) / 2.0 ** -53
    d = ulp_distance(got, want)
    if kind == "stab":
        return d / np.maximum(1.0, 0.5 * ((z - p1) / p2) ** 2)
    return d


FUNC_BOUND = {"": 4, "logit": 4, "probit": 2, "stab": 4}


def test_selection_values_at_scale_follow_the_reference_arithmetic(gpu_lib, oracle_lib):
    """ve = 0 for every phenotype, so the device's and the oracle's phenotypes are bit-identical; the values are then computed
    from the ORACLE's phenotypes (mv, sv in phenotype order, :3310-3318): mating values bit for bit, the generation-0 mean and
    variance within the tree-sum bound of the exact ones, z within the bound that follows, every selection function at the device's
    own z against the C formula (libm correctly rounded), thr exact including z == thr, and the couples of random_mate_selected
    equal to the oracle's random_mate on the downloaded values, with about a third of them NaN (logit overflow)"""
    n = N_BIG
    g, o = twins(gpu_lib, oracle_lib, n)
    rng = np.random.default_rng(5)
    cs = rng.standard_normal(n) * 0.2
    par = [(0.5, 0.2, 0.0, 0.0, None), (0.6, -1.0, 0.0, 0.0, cs), (-1.0, 0.1, 0.0, 0.0, None)]
    phens = []
    for p, (va, vd, ve, vf, c) in enumerate(par):
        dev = gef(g, p, 0, 99 + p, va, vd, ve, vf, cs=c)["phen"]
        ora = gef(o, p, 0, 99 + p, va, vd, ve, vf, cs=c)["phen"]
        assert first_bit_difference(dev, ora) is None, f"phenotype {p}: ve = 0 phenotypes are bit-identical"
        phens.append(ora)
    omega, lam = [1.0, -0.5, 0.25], [1.0, 0.7, -1.2]
    mv, sv = np.zeros(n), np.zeros(n)
    for p in range(3):
        mv = mv + omega[p] * phens[p]
        sv = sv + lam[p] * phens[p]
    d0 = g.compute_selection(0, 0, "none", 0, 0, omega, lam)
    diff = first_bit_difference(d0["mating_value"], mv)
    assert diff is None, f"mating values: first difference at {diff[0]}"
    # generation-0 statistics: tree sums of k = ceil(n / 65536) terms per thread, then 8 + 8 levels
    k = math.ceil(n / 65536)
    m_ex, v_ex = exact_mean_var(sv)
    m_dev, v_dev = g.get_selection_gen0(0)
    dm = (k + 18) * EPS * float(np.sum(np.abs(sv))) / n + EPS * abs(m_ex)
    assert abs(m_dev - m_ex) <= dm, f"generation-0 mean {m_dev!r}, exact {m_ex!r}, bound {dm}"
    dv = (k + 20) * EPS * v_ex + n * dm * dm / (n - 1)
    assert abs(v_dev - v_ex) <= dv, f"generation-0 variance {v_dev!r}, exact {v_ex!r}, bound {dv}"
    record("gen0 mean / var error in eps", (abs(m_dev - m_ex) / (EPS * float(np.sum(np.abs(sv))) / n), abs(v_dev - v_ex) / (EPS * v_ex)))
    sigma = math.sqrt(v_ex)
    z_ex = (sv - m_ex) / sigma
    bz = (dm + EPS * np.abs(sv - m_ex)) / sigma + np.abs(z_ex) * ((k + 20) / 2 + 3) * EPS
    for gen, z in ((0, d0["selection_value"]), (1, g.compute_selection(0, 1, "none", 0, 0, omega, lam)["selection_value"])):
        i = int(np.argmax(np.abs(z - z_ex) - bz))
        assert abs(z[i] - z_ex[i]) <= bz[i], f"generation {gen}: z at {i} is {z[i]!r}, exact {z_ex[i]!r}, bound {bz[i]}"
    z = d0["selection_value"]
    thr = float(z[123])
    sample = np.unique(np.r_[rng.choice(n, 20000, replace=False), np.argsort(z)[:50], np.argsort(z)[-50:], 123])
    worst = []
    for kind, p1, p2 in FUNCS_E:
        p2 = thr if kind == "thr" else p2
        got = g.compute_selection(0, 1, kind, p1, p2, omega, lam)
        assert first_bit_difference(got["selection_value"], z) is None, "z does not depend on the function"
        svf = got["selection_value_func"]
        mirror = ras_selection_func(1, kind, p1, p2, z)
        assert np.array_equal(np.isnan(svf), np.isnan(mirror)), f"{kind!r}: NaN pattern differs from C's"
        if kind in ("thr", "none"):
            assert first_bit_difference(svf, mirror) is None, f"{kind!r}: not bit-identical"
            if kind == "thr":
                assert svf[123] == 0.4 and (svf == 0.4).sum() == (z <= thr).sum(), "z == thr gives p1"
            continue
        want = c_selection_formula(kind, p1, p2, z[sample])
        err = func_error(kind, p1, p2, svf[sample], want, z[sample])
        j = int(np.argmax(err))
        record(f"selection function {kind!r} {p1} {p2}", float(err[j]))
        worst.append((float(err[j]), kind, p1, p2, float(z[sample][j]), float(svf[sample][j]), float(want[j])))
    for e, kind, p1, p2, zj, a, b in worst:
        assert e <= FUNC_BOUND[kind], f"{kind!r} {p1} {p2}: at z = {zj!r} the device gives {a!r}, C {b!r} (error {e})"
    # mating on the device's values against the oracle's random_mate on the same values downloaded, a third of them NaN
    b1 = 709.8 / float(np.quantile(z, 2 / 3))
    svf = g.compute_selection(0, 1, "logit", 0.0, b1, omega, lam)["selection_value_func"]
    assert 0.3 * n < np.isnan(svf).sum() < 0.37 * n
    for seed, pop_size in ((4242, n), (999_983, n // 2 + 7)):
        cg, mg, fg = g.random_mate_selected(0, seed, pop_size)
        co, mo, fo = o.random_mate(0, seed, svf, pop_size)
        assert (mg, fg) == (mo, fo), f"mating counts differ: device {(mg, fg)}, oracle {(mo, fo)}"
        bad = np.flatnonzero(cg != co)
        assert len(bad) == 0, f"couples differ at {bad[:5]} (seed {seed}, {pop_size} couples)"
        assert not np.isnan(svf[cg["pos_male"].astype(np.int64)]).any() and not np.isnan(svf[cg["pos_female"].astype(np.int64)]).any()
    g.close(); o.close()


# ---- f. edge inputs on the device -----------------------------------------------------------------------------------------------
EDGES = [("logit", 0.0, 1000.0), ("stab", 0.0, 1e-200), ("stab", 0.0, 0.0), ("probit", 0.0, 0.0), ("probit", 0.5, 0.0)]


@pytest.mark.parametrize("kind,p1,p2", EDGES, ids=["logit-b1-1000", "stab-sigma-1e-200", "stab-sigma-0", "probit-sigma-0", "probit-sigma-0-mu-half"])
def test_edge_inputs_give_what_c_gives(gpu_lib, oracle_lib, kind, p1, p2):
    """the device at the inputs where the formulas overflow or divide by zero gives what the reference's C gives under glibc (the
    host mirror, and the same values written out: 1/0 = inf, 0/0 = NaN, erf(+-inf) = +-1, exp(-inf) = 0, inf * 0 = NaN).  z is set
    exactly: phenotype 0 = raw additive / 1 (va = -1), nothing else, standardised with mean 0 and variance 0 (z = sv - 0)."""
    zs = np.array([1.0, 0.0, -2.0, 0.5, 0.25, -0.0625, 3.0, 0.7109375])
    n = len(zs)
    a = np.stack([zs, np.ones(n), np.ones(n)], axis=1)
    g, o = twins(gpu_lib, oracle_lib, n, a=a, d=np.zeros((n, 3)))
    o.close()
    for p in range(3):
        assert first_bit_difference(gef(g, p, 0, 7 + p, -1.0, 0.0, 0.0, 0.0)["phen"], a[:, p]) is None
    g.compute_selection(0, 0, "none", 0, 0, [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], want=())
    g.set_selection_gen0(0, 0.0, 0.0)
    got = g.compute_selection(0, 1, kind, p1, p2, [1.0, 0.0, 0.0], [1.0, 0.0, 0.0])
    assert first_bit_difference(got["selection_value"], zs) is None
    svf = got["selection_value_func"]
    for want, what in ((ras_selection_func(1, kind, p1, p2, zs), "host mirror"), (c_selection_formula(kind, p1, p2, zs), "C formula")):
        assert np.array_equal(np.isnan(svf), np.isnan(want)), f"{kind} {p1} {p2}: NaN pattern differs from the {what}: {svf} vs {want}"
        ok = ~np.isnan(want)
        assert np.array_equal(svf[ok], want[ok]), f"{kind} {p1} {p2}: values differ from the {what}: {svf} vs {want}"
    if kind == "logit":
        assert np.array_equal(np.isnan(svf), zs * 1000.0 > 709.78), "NaN exactly where exp(1000 z) overflows"
    elif kind == "stab":
        assert np.isnan(svf).all() if p2 == 0.0 else (np.array_equal(svf == 0.0, zs != 0.0) and svf[zs == 0.0][0] > 1e199)
    else:
        assert np.array_equal(np.isnan(svf), zs == p1) and np.array_equal(svf[zs > p1], np.ones((zs > p1).sum())) and (svf[zs < p1] == 0.0).all()
    g.close()
