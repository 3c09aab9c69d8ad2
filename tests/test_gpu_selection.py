"""Mating and selection values on the device (gev_compute_selection) fed straight into the next generation
(gev_generation_begin_selected / gev_random_mate_selected): closed loops against the reference's fixtures, at scale against the
host mirror, and the edge cases of Simulation::ras_compute_mating_value_selection_value / ras_selection_func
(reference src/Simulation.cpp:3300-3342, :3386-3428)."""
import numpy as np
import pytest

from geneevolve_amd import capi
from geneevolve_amd.host import (Simulation, SyntheticConfig, NormalEngine, SampleWithoutReplacement, comm_mean, comm_var,
                                 environmental_effects_specific_to_each_population, ras_do_migration, ras_selection_func, random_mate)
from tests import helpers

pytestmark = pytest.mark.gpu

RTOL = 1e-12                        # device libm and parallel sums against glibc and sequential sums (as the device-GEF tests)


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern"
    ok = ~np.isnan(a)
    assert np.allclose(a[ok], b[ok], rtol=RTOL, atol=1e-13), f"{what}: max abs diff {np.max(np.abs(a[ok] - b[ok]), initial=0)}"


def couples_equal(c, want):
    return len(c) == len(want) and np.array_equal(c["pos_male"].astype(np.int64), want[:, 0]) and np.array_equal(c["pos_female"].astype(np.int64), want[:, 1])


def host_values(phens, omega, lam, gen_num, func, p1, p2, sv0):
    """the host mirror: mv / sv in phenotype order, standardised to generation 0, ras_selection_func"""
    mv = np.zeros(len(phens[0])); sv = np.zeros(len(phens[0]))
    for p, ph in enumerate(phens):
        mv = mv + omega[p] * ph; sv = sv + lam[p] * ph
    if gen_num == 0:
        sv0 = (comm_mean(sv), comm_var(sv))
    z = (sv - sv0[0]) / np.sqrt(sv0[1]) if sv0[1] > 0 else sv - sv0[0]
    return mv, z, ras_selection_func(gen_num, func, p1, p2, z), sv0


# ---- 1. closed loops on the reference's random-mating fixtures, no host svf -----------------------------------------------------
@pytest.mark.parametrize("case", ["sel1", "syn1k", "vt2", "om1"])
def test_closed_loop_with_device_selection_values_matches_reference_fixture(gpu_lib, case):
    fx = helpers.load_fixture(case)
    assert int(fx["n_pop"]) == 1
    nchr, nphen, ngen, rm = int(fx["nchr"]), int(fx["nphen"]), int(fx["n_gen"]), bool(int(fx["pop0_rm"]))
    ctx = gpu_lib.create(1, nchr, nphen)
    helpers.setup_static(ctx, fx)
    var = [[float(v) for v in fx[f"pop0_ph{p}_var"]] for p in range(nphen)]
    vc = [float(fx[f"pop0_ph{p}_vc"]) if f"pop0_ph{p}_vc" in fx else 0.0 for p in range(nphen)]
    omega = [float(fx[f"pop0_ph{p}_omega"]) if f"pop0_ph{p}_omega" in fx else 1.0 for p in range(nphen)]
    lam = [float(fx[f"pop0_ph{p}_lambda"]) if f"pop0_ph{p}_lambda" in fx else 1.0 for p in range(nphen)]
    extra = [str(x) for x in fx["args_extra"]]
    vt_type = int(extra[extra.index("--vt_type") + 1]) if "--vt_type" in extra else 1
    handed_down = "phen" if vt_type == 1 else "parental_effect"
    mm = float(extra[extra.index("--MM") + 1]) if "--MM" in extra else 0.0
    avoid = "--avoid_inbreeding" in extra
    sim = Simulation(ctx, int(fx["seed"]), nchr, bool(int(fx["pop0_has_mut"])), track_pedigree=True)
    beta = [1.0] * nphen

    def scale(g, s2, prev, common):
        n = len(sim.sex[0]); outs = []
        for p in range(nphen):
            va, vd, ve, vf = var[p]
            seed = int(sim.ras_glob_seed()[0])
            ff = prev[p][sim.ped[0].ID_Father] if g > 0 else np.zeros(n)
            fm = prev[p][sim.ped[0].ID_Mother] if g > 0 else np.zeros(n)
            o = ctx.scale_ad_compute_gef(0, p, g, seed, va, vd, ve, vf, beta[p], s2[p][0], s2[p][1], common_sibling=common[p], f_father=ff, f_mother=fm)
            if g > 0:
                assert seed == int(fx[f"g{g}_pop0_ph{p}_gef_seed"]), f"{case}: ras_glob_seed() stream out of step at generation {g}"
                close(o["phen"], fx[f"g{g}_pop0_ph{p}_gef_out"][:, 5], f"{case}: phenotype {p} generation {g}")
            outs.append(o)
        return outs

    sim.ras_initial_human_gen0(0, len(fx["g0_pop0_sex"]))
    n0 = len(sim.sex[0])
    common0 = [NormalEngine(int(sim.ras_glob_seed()[0])).draw(n0, float(np.sqrt(vc[p]))) if vc[p] > 0 else np.zeros(n0) for p in range(nphen)]
    add, dom, _, _ = ctx.compute_ad(0)
    s2 = [(comm_var(add[:, p]), comm_var(dom[:, p])) for p in range(nphen)]
    outs = scale(0, s2, None, common0)
    dev = ctx.compute_selection(0, 0, "none", 0, 0, omega, lam)
    mv, z, svf, sv0 = host_values([o["phen"] for o in outs], omega, lam, 0, None, 0, 0, None)
    close(ctx.get_selection_gen0(0), sv0, f"{case}: generation-0 mean / variance of the selection value")
    close(dev["mating_value"], mv, f"{case}: mating values generation 0"); close(dev["selection_value"], z, f"{case}: selection values generation 0")
    assert np.array_equal(dev["selection_value_func"], np.ones(n0))
    for p in range(nphen):                                               # "adjust beta" (:648-657)
        if vt_type == 1:
            beta[p] = float(np.sqrt(var[p][3] / (2 * comm_var(outs[p]["phen"]))))
        elif comm_var(outs[p]["parental_effect"]) > 0:
            beta[p] = float(np.sqrt(var[p][3] / (2 * comm_var(outs[p]["parental_effect"]))))
    for g in range(1, ngen + 1):
        pop_size, mat_cor, dist, func, p1, p2 = str(fx["pop0_popinfo"][g - 1]).split()
        k = f"g{g}_pop0_mate_"
        close(dev["selection_value_func"], fx[k + "svf"], f"{case}: selection function values entering generation {g}")
        prev = [o[handed_down] for o in outs]
        if rm:
            res = sim.next_generation_rm_selected(0, int(pop_size), want_couples=True)
            assert int(res["seed_mate"]) == int(fx[k + "seed"]) and int(res["seed_reproduce"]) == int(fx[f"g{g}_pop0_seed_reproduce"])
        else:                                                            # om1: the device's values feed the host's assort_mate
            close(dev["mating_value"], fx[k + "am_mv"], f"{case}: mating values entering generation {g}")
            sim.assort_mate(0, dev["selection_value_func"], dev["mating_value"], int(pop_size), float(mat_cor), mm_percent=mm,
                            avoid_inbreeding=avoid, offspring_dist=dist, rank=ctx.rank_f64)
        want = fx[f"g{g}_pop0_couples"]
        c = sim.couples[0]
        assert couples_equal(c, want) and np.array_equal(c["inbreed"], want[:, 2]) and np.array_equal(c["num_offspring"], want[:, 3]), f"{case}: couples of generation {g}"
        if not rm:
            sim.reproduce(0, g)
        assert np.array_equal(sim.sex[0], fx[f"g{g}_pop0_sex"]), f"{case}: sex generation {g}"
        ped = sim.ped[0]
        assert np.array_equal(np.stack([ped.ID, ped.ID_Father, ped.ID_Mother], axis=1), fx[f"g{g}_pop0_ids"]), f"{case}: pedigree generation {g}"
        with pytest.raises(capi.GevError) as e:                          # the published generation dropped the values of the parents
            ctx.download_selection(0)
        assert e.value.code == -2
        n = len(sim.sex[0])
        common = sim.common_sibling(0, vc) if any(v > 0 for v in vc) else [np.zeros(n)] * nphen
        outs = scale(g, s2, prev, common)
        dev = ctx.compute_selection(0, g, func, float(p1), float(p2), omega, lam)
        mv, z, svf, _ = host_values([o["phen"] for o in outs], omega, lam, g, func, float(p1), float(p2), sv0)
        close(dev["mating_value"], mv, f"{case}: mating values generation {g}")
        close(dev["selection_value"], z, f"{case}: selection values generation {g}")
        close(dev["selection_value_func"], svf, f"{case}: selection function values generation {g}")
    ctx.close()


# ---- 2. two populations, --gamma, in-context migration ------------------------------------------------------------------------
def test_gamma_and_migration_fixture_with_device_selection_values(gpu_lib):
    fx = helpers.load_fixture("gam2")
    n_pop, nchr, ngen = int(fx["n_pop"]), int(fx["nchr"]), int(fx["n_gen"])
    assert int(fx["nphen"]) == 1
    extra = [str(x) for x in fx["args_extra"]]
    gamma = float(extra[extra.index("--gamma") + 1])
    ctx = gpu_lib.create(n_pop, nchr, 1)
    helpers.setup_static(ctx, fx)
    sim = Simulation(ctx, int(fx["seed"]), nchr, bool(int(fx["pop0_has_mut"])), track_pedigree=True)
    sampler = SampleWithoutReplacement()
    var = [[float(v) for v in fx[f"pop{ip}_ph0_var"]] for ip in range(n_pop)]
    s2, sv0, host = [None] * n_pop, [None] * n_pop, [None] * n_pop

    def scale(ip, g):
        n = len(sim.sex[ip]); va, vd, ve, vf = var[ip]
        seed = int(sim.ras_glob_seed()[0])
        o = ctx.scale_ad_compute_gef(ip, 0, g, seed, va, vd, ve, vf, 1.0, s2[ip][0], s2[ip][1], common_sibling=np.zeros(n), f_father=np.zeros(n), f_mother=np.zeros(n))
        if g > 0:
            close(o["phen"], fx[f"g{g}_pop{ip}_ph0_gef_out"][:, 5], f"phenotypes gen {g} pop {ip}")
        return o["phen"]

    def selection(g, phens, funcs):
        shifted = [ph.copy() for ph in phens]
        a = environmental_effects_specific_to_each_population(shifted, gamma)
        for ip in range(n_pop):
            shift = a * float((2 * ip) // (n_pop - 1) - 1)                # what the reference adds to Human::phen (:3291)
            f = funcs[ip] if g > 0 else ("none", 0.0, 0.0)
            dev = ctx.compute_selection(ip, g, f[0], f[1], f[2], [1.0], [1.0], phen_shift=[shift])
            mv, z, svf, s = host_values([shifted[ip]], [1.0], [1.0], g, f[0], f[1], f[2], sv0[ip])
            sv0[ip] = s
            close(dev["mating_value"], mv, f"mating values gen {g} pop {ip}")
            close(dev["selection_value"], z, f"selection values gen {g} pop {ip}")
            close(dev["selection_value_func"], svf, f"selection function values gen {g} pop {ip}")
            host[ip] = {"mv": mv, "z": z, "svf": svf}

    phens = []
    for ip in range(n_pop):
        sim.ras_initial_human_gen0(ip, len(fx[f"g0_pop{ip}_sex"]))
        add, dom, _, _ = ctx.compute_ad(ip)
        s2[ip] = (comm_var(add[:, 0]), comm_var(dom[:, 0]))
        phens.append(scale(ip, 0))
    selection(0, phens, None)
    for g in range(1, ngen + 1):
        funcs, phens = [], []
        for ip in range(n_pop):
            pop_size, _, _, func, p1, p2 = str(fx[f"pop{ip}_popinfo"][g - 1]).split()
            funcs.append((func, float(p1), float(p2)))
            close(host[ip]["svf"], fx[f"g{g}_pop{ip}_mate_svf"], f"selection function values entering gen {g} pop {ip}")
            sim.next_generation_rm_selected(ip, int(pop_size), want_couples=True)
            assert couples_equal(sim.couples[ip], fx[f"g{g}_pop{ip}_couples"]), f"couples gen {g} pop {ip}"
            assert np.array_equal(sim.sex[ip], fx[f"g{g}_pop{ip}_sex"]), f"sex gen {g} pop {ip}"
            phens.append(scale(ip, g))
        selection(g, phens, funcs)
        moves = ras_do_migration([len(sim.sex[ip]) for ip in range(n_pop)], fx["migration_mat_gen"][g - 1], sim.ras_glob_seed, sampler)
        assert moves == helpers.derive_moves(fx, g), f"WHO migrates in generation {g}"
        sim.ras_do_migration(moves)
        gone = [np.zeros(len(sim.sex[ip]), dtype=bool) for ip in range(n_pop)]
        for sp, pos, dp in moves:
            gone[sp][pos] = True
        old = [(sim.sex[ip], sim.ped[ip], host[ip]) for ip in range(n_pop)]
        for ip in range(n_pop):                                          # the host's records follow the migrants
            keep = np.flatnonzero(~gone[ip])
            sx, pd, r = old[ip]
            sex_new, ped_new = [sx[keep]], pd.take(keep)
            cols = {k: [r[k][keep]] for k in r}
            for sp, pos, dp in moves:
                if dp == ip:
                    sex_new.append(old[sp][0][pos:pos + 1]); ped_new = ped_new.append(old[sp][1].take(np.array([pos])))
                    for k in cols:
                        cols[k].append(old[sp][2][k][pos:pos + 1])
            sim.sex[ip], sim.ped[ip] = np.concatenate(sex_new), ped_new
            host[ip] = {k: np.concatenate(v) for k, v in cols.items()}
            assert np.array_equal(sim.sex[ip], fx[f"g{g}_pop{ip}_postmig_sex"]), f"post-migration sex gen {g} pop {ip}"
        for ip in range(n_pop):                                          # the device's values followed them too
            d = ctx.download_selection(ip)
            close(d["mating_value"], host[ip]["mv"], f"post-migration mating values gen {g} pop {ip}")
            close(d["selection_value"], host[ip]["z"], f"post-migration selection values gen {g} pop {ip}")
            close(d["selection_value_func"], host[ip]["svf"], f"post-migration selection function values gen {g} pop {ip}")
    ctx.close()


# ---- 3. at scale: 100k individuals, synthetic inputs ---------------------------------------------------------------------------
N_SCALE = 100_000
FUNCS = [("", 0.0, 0.0), ("logit", 1.0, 1.0), ("probit", -0.3, 0.8), ("stab", 0.2, 1.3), ("thr", 0.4, 0.25), ("none", 0.0, 0.0)]


def scale_context(gpu_lib, nphen, seed=5):
    cfg = SyntheticConfig(N_SCALE, 4096, chrom_bp=20_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=200, nphen=nphen, seed=seed)
    ctx = gpu_lib.create(1, 1, nphen)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * N_SCALE, seed + 1)
    for p in range(nphen):
        ctx.synth_cv_founders(0, p, 0, 2 * N_SCALE, seed + 10 + p)
    sim = Simulation(ctx, 1000 + seed, 1, True)
    sim.ras_initial_human_gen0(0, N_SCALE)
    return ctx, sim


def gef_all(ctx, sim, g, nphen, s2=None):
    if s2 is None:
        add, dom, _, _ = ctx.compute_ad(0, per_chr=False)
        s2 = [(comm_var(add[:, p]), comm_var(dom[:, p])) for p in range(nphen)]
    phens = [ctx.scale_ad_compute_gef(0, p, g, int(sim.ras_glob_seed()[0]), 0.4 + 0.1 * p, 0.0, 0.5, 0.0, 1.0, s2[p][0], s2[p][1])["phen"] for p in range(nphen)]
    return phens, s2


@pytest.mark.parametrize("nphen", [1, 3])
def test_device_values_equal_the_host_mirror_at_scale(gpu_lib, nphen):
    ctx, sim = scale_context(gpu_lib, nphen)
    omega, lam = [1.0, -0.5, 0.25][:nphen], [1.0, 0.7, -1.2][:nphen]
    phens, s2 = gef_all(ctx, sim, 0, nphen)
    dev = ctx.compute_selection(0, 0, "none", 0, 0, omega, lam)
    mv, z, _, sv0 = host_values(phens, omega, lam, 0, None, 0, 0, None)
    close(ctx.get_selection_gen0(0), sv0, "generation-0 statistics")
    close(dev["mating_value"], mv, "mating values"); close(dev["selection_value"], z, "selection values")
    for func, p1, p2 in FUNCS:
        dev = ctx.compute_selection(0, 1, func, p1, p2, omega, lam)
        mv, z, svf, _ = host_values(phens, omega, lam, 1, func, p1, p2, sv0)
        close(dev["mating_value"], mv, f"{func!r}: mating values"); close(dev["selection_value"], z, f"{func!r}: selection values")
        close(dev["selection_value_func"], svf, f"{func!r}: selection function values")
    ctx.close()


@pytest.mark.parametrize("nphen", [1, 3])
@pytest.mark.parametrize("head_start", [False, True])
def test_selected_generation_gives_the_couples_of_the_uploaded_values_at_scale(gpu_lib, nphen, head_start):
    """two identical contexts: one mates on the device's values, the other on the same values downloaded and handed back"""
    runs = []
    for mode in ("device", "host"):
        ctx, sim = scale_context(gpu_lib, nphen, seed=7)
        if head_start:
            ctx.set_generation_chain(nphen)                  # between two generations: one ras_glob_seed() per phenotype (GEF, :3078)
        omega, lam = [1.0, 0.5, -0.25][:nphen], [1.0, -0.6, 0.9][:nphen]
        phens, s2 = gef_all(ctx, sim, 0, nphen)
        dev = ctx.compute_selection(0, 0, "none", 0, 0, omega, lam, want=("selection_value_func",) if mode == "host" else ())
        out = []
        for g in range(1, 4):
            if mode == "device":
                r = sim.next_generation_rm_selected(0, N_SCALE, want_couples=True)
            else:
                r = sim.next_generation_rm(0, N_SCALE, dev["selection_value_func"], want_couples=True)
            out.append((r["couples"].copy(), r["sex"].copy(), int(r["glob_state"])))
            phens, _ = gef_all(ctx, sim, g, nphen, s2)
            func, p1, p2 = FUNCS[g % len(FUNCS)][0:3] if g != 3 else ("logit", 1.0, 1.0)
            dev = ctx.compute_selection(0, g, func, p1, p2, omega, lam, want=("selection_value_func",) if mode == "host" else ())
        runs.append(out)
        ctx.close()
    for g, (a, b) in enumerate(zip(*runs), start=1):
        assert np.array_equal(a[0], b[0]), f"couples generation {g}"
        assert np.array_equal(a[1], b[1]) and a[2] == b[2], f"sexes / engine state generation {g}"


# ---- 4. edge cases -------------------------------------------------------------------------------------------------------------
def small_context(gpu_lib, n=2000, seed=11):
    cfg = SyntheticConfig(n, 2048, chrom_bp=2_000_000, map_step=10_000, rec_per_row=1e-3, mut_per_row=1e-3, n_cv=64, seed=seed)
    ctx = gpu_lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, seed + 1); ctx.synth_cv_founders(0, 0, 0, 2 * n, seed + 2)
    sim = Simulation(ctx, 77 + seed, 1, True)
    sim.ras_initial_human_gen0(0, n)
    return ctx, sim


def test_logit_overflow_gives_nan_and_that_individual_never_mates(gpu_lib):
    ctx, sim = small_context(gpu_lib)
    phens, _ = gef_all(ctx, sim, 0, 1)
    ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0], want=())
    dev = ctx.compute_selection(0, 1, "logit", 0.0, 1000.0, [1.0], [1.0])
    svf = dev["selection_value_func"]
    nan = np.isnan(svf)
    assert 0.1 * len(svf) < nan.sum() < 0.9 * len(svf), "exp(b0 + b1*z) overflows for the individuals above z = 0.71"
    with np.errstate(over="ignore"):
        assert np.array_equal(nan, np.isinf(np.exp(0.0 + 1000.0 * dev["selection_value"]))), "NaN exactly where exp overflows"
    couples, nm, nf = ctx.random_mate_selected(0, 12345, len(svf))
    assert not nan[couples["pos_male"].astype(np.int64)].any() and not nan[couples["pos_female"].astype(np.int64)].any(), "an individual with NaN mated"
    want = random_mate(sim.sex[0], svf, len(svf), 12345)                 # the host mirror of Simulation::random_mate on the same values
    assert np.array_equal(couples["pos_male"], want["pos_male"]) and np.array_equal(couples["pos_female"], want["pos_female"])
    ctx.close()


def test_zero_generation0_variance_uses_the_undivided_branch(gpu_lib):
    ctx, sim = small_context(gpu_lib)
    phens, _ = gef_all(ctx, sim, 0, 1)
    ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [0.0], want=())  # lambda 0: sv = 0 for all, var 0
    assert ctx.get_selection_gen0(0) == (0.0, 0.0)
    dev = ctx.compute_selection(0, 1, "logit", 0.0, 1.0, [1.0], [1.0])
    assert np.array_equal(dev["selection_value"], phens[0] - 0.0), "z = sv - mean when the generation-0 variance is 0"
    ctx.set_selection_gen0(0, 0.25, 0.0)
    dev = ctx.compute_selection(0, 1, "thr", 0.5, 0.1, [1.0], [1.0])
    assert np.array_equal(dev["selection_value"], phens[0] - 0.25)
    assert np.array_equal(dev["selection_value_func"], np.where(phens[0] - 0.25 <= 0.1, 0.5, 1.0))
    ctx.close()


def test_none_and_generation0_give_ones_and_the_couples_of_no_values(gpu_lib):
    ctx, sim = small_context(gpu_lib)
    gef_all(ctx, sim, 0, 1)
    n = ctx.pop_size(0)
    dev = ctx.compute_selection(0, 0, "logit", 5.0, -3.0, [1.0], [1.0])   # generation 0: 1 for all whatever the function
    assert np.array_equal(dev["selection_value_func"], np.ones(n))
    ref, _, _ = ctx.random_mate(0, 999, None, n)
    got, _, _ = ctx.random_mate_selected(0, 999, n)
    assert np.array_equal(got, ref)
    dev = ctx.compute_selection(0, 3, "none", 5.0, -3.0, [1.0], [1.0])
    assert np.array_equal(dev["selection_value_func"], np.ones(n))
    got, _, _ = ctx.random_mate_selected(0, 999, n)
    assert np.array_equal(got, ref)
    ctx.close()


def test_selected_calls_are_refused_without_current_values(gpu_lib):
    import torch
    ctx, sim = small_context(gpu_lib)
    n = ctx.pop_size(0)
    with pytest.raises(capi.GevError) as e:
        ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0])      # no phenotypes yet
    assert e.value.code == -2
    gef_all(ctx, sim, 0, 1)
    with pytest.raises(capi.GevError) as e:
        ctx.compute_selection(0, 1, "logit", 1, 1, [1.0], [1.0])     # no generation-0 statistics yet
    assert e.value.code == -2
    for call in (lambda: ctx.generation_begin_selected(0, sim.glob.x, n), lambda: ctx.random_mate_selected(0, 1, n)):
        with pytest.raises(capi.GevError) as e:
            call()
        assert e.value.code == -2
    ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0], want=())
    sim.next_generation_rm_selected(0, n)                                 # publishes a generation: its parents' values are gone
    for call in (lambda: ctx.generation_begin_selected(0, sim.glob.x, n), lambda: ctx.random_mate_selected(0, 1, n), lambda: ctx.download_selection(0)):
        with pytest.raises(capi.GevError) as e:
            call()
        assert e.value.code == -2 and "selection values" in str(e.value)
    gef_all(ctx, sim, 1, 1, [(1.0, 0.0)])
    ctx.compute_selection(0, 1, "logit", 1, 1, [1.0], [1.0], want=())
    ctx.random_mate_selected(0, 1, n)                                     # valid again
    who = np.array([3, 17], dtype=np.uint64)
    nb = ctx.export_size(0, who)
    buf = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ctx.export_rows(0, who, buf.data_ptr(), nb)
    torch.cuda.synchronize()
    ctx.remove_rows(0, np.array([5, 9], dtype=np.uint64)); ctx.import_rows(0, buf.data_ptr(), nb, 2)
    assert ctx.pop_size(0) == n
    with pytest.raises(capi.GevError) as e:
        ctx.random_mate_selected(0, 1, n)
    assert e.value.code == -2
    ctx.close()
    del buf


def test_set_generation0_statistics_match_the_self_computed_ones(gpu_lib):
    ctx, sim = small_context(gpu_lib)
    gef_all(ctx, sim, 0, 1)
    ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0], want=())
    m, v = ctx.get_selection_gen0(0)
    a = ctx.compute_selection(0, 2, "probit", 0.1, 0.9, [1.0], [1.0])
    ctx.set_selection_gen0(0, 0.0, 1.0)
    b = ctx.compute_selection(0, 2, "probit", 0.1, 0.9, [1.0], [1.0])
    assert not np.array_equal(a["selection_value"], b["selection_value"])
    ctx.set_selection_gen0(0, m, v)
    b = ctx.compute_selection(0, 2, "probit", 0.1, 0.9, [1.0], [1.0])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    ctx.close()
