"""A generation's phenotypes from state the library holds.  First half: the pedigree ids of reference `class Human` kept on the device
(gev_set_track_pedigree, reference src/Simulation.cpp:2473-2479, :3037-3043): closed loops and replays of the fixtures with tracking
on, assortative generations whose inbreeding test reads the device's ids, migration, rows removed / imported, the host mirror at
size, the refusals; everything there is integer: exact.  Second half: gev_generation_phenotypes / gev_phenotypes_result /
gev_save_prev_gen (ras_scale_AD_compute_GEF of every phenotype, :3075-3206, with the family effects of :2417-2429 and the gather by id
of :3118-3131): closed loops from --seed alone with nothing uploaded after generation 0, one step against the reference's recorded
inputs, migration, the head start, the forced rerun, 100 000 individuals against the host mirror, the refusals.  Tolerances: 1e-12
relative for one device step (tests/test_gpu_selection.py:RTOL), rtol 1e-9 / atol 1e-12 for floats carried through a closed loop."""
import ctypes as C

import numpy as np
import pytest

from geneevolve_amd import capi, host
from geneevolve_amd.host import NormalEngine, Pedigree, Simulation, SyntheticConfig, comm_var
from tests import helpers
from tests.test_gpu_selection import close

pytestmark = pytest.mark.gpu


def ped_records(P):
    return np.stack([getattr(P, f) for f in Pedigree.FIELDS], axis=1).astype(np.int64)


class TrackedSimulation(Simulation):
    """the host mirror keeps its own pedigree (as the closed loops of tests/helpers.py ask) AND the library tracks the ids: compared,
    all seven fields of every population, before and after every step that publishes a generation, and when the context closes"""

    def __init__(self, ctx, seed, nchr, has_mutation_map, track_pedigree=True):
        super().__init__(ctx, seed, nchr, has_mutation_map, track_pedigree=True, device_pedigree=True)
        ctx._tracked_sim = self
        self.n_compared = 0

    def compare(self, where):
        for ip, P in self.ped.items():
            got = self.ctx.download_pedigree(ip)
            assert np.array_equal(got, ped_records(P)), f"device pedigree ids of population {ip} differ from the host mirror's {where}"
            self.n_compared += 1

    def reproduce(self, ipop, *a, **k):
        self.compare(f"before reproduce({ipop})")
        r = super().reproduce(ipop, *a, **k)
        self.compare(f"after reproduce({ipop})")
        return r

    def next_generation_rm(self, ipop, *a, **k):
        self.compare(f"before the generation of population {ipop}")
        r = super().next_generation_rm(ipop, *a, **k)
        self.compare(f"after the generation of population {ipop}")
        return r

    def next_generation_am(self, ipop, *a, **k):
        self.compare(f"before the assortative generation of population {ipop}")
        r = super().next_generation_am(ipop, *a, **k)
        self.compare(f"after the assortative generation of population {ipop}")
        return r


class TrackedLibrary:
    """the library with contexts that compare once more when the closed loop closes them (behind the last generation's migration)"""

    def __init__(self, lib):
        self._lib = lib
        self.n_compared = 0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def create(self, *args):
        ctx = self._lib.create(*args)
        real_close, outer = ctx.close, self

        def close_checked():
            sim = getattr(ctx, "_tracked_sim", None)
            if sim is not None and ctx.h:
                ctx._tracked_sim = None
                sim.compare("at the end of the run")
                outer.n_compared += sim.n_compared
            real_close()
        ctx.close = close_checked
        return ctx


# ---- 1. closed loops from --seed alone, tracking on ------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mate", [("am1", "host"), ("am2", "host"), ("vc1", "host"), ("dense", "host"), ("dense", "device"), ("dense", "fused"), ("vt2", "fused")])
def test_device_pedigree_through_closed_loops(gpu_lib, monkeypatch, case, mate):
    """the closed loop of tests/helpers.py (which compares the host mirror's ID, ID_Father, ID_Mother with the fixture's every
    generation) with the library tracking the ids: host couples (am1: second spouses, avoid_inbreeding, Poisson families), couples
    left by gev_random_mate, whole generations of gev_generation_begin"""
    monkeypatch.setattr(host, "Simulation", TrackedSimulation)
    lib = TrackedLibrary(gpu_lib)
    fx = helpers.load_fixture(case)
    helpers.closed_loop_case(lib, fx, f"gpu/{case}/{mate}/tracked", device=0, exact=False, mate=mate)
    assert lib.n_compared >= 2 * int(fx["n_gen"]) + 1


@pytest.mark.parametrize("mate", ["host", "fused"])
def test_device_pedigree_follows_the_migrants(gpu_lib, monkeypatch, mate):
    """mig2 from the seed alone: gev_migrate carries the ids as it carries the selection values; the loop itself compares the host
    mirror with the fixture's post-migration ids"""
    monkeypatch.setattr(host, "Simulation", TrackedSimulation)
    lib = TrackedLibrary(gpu_lib)
    fx = helpers.load_fixture("mig2")
    helpers.closed_loop_migration_case(lib, fx, f"gpu/mig2/{mate}/tracked", device=0, exact=False, mate=mate)
    assert lib.n_compared >= 4 * int(fx["n_gen"])


def test_device_pedigree_replay_of_unequal_migration(gpu_lib, oracle_lib):
    """mig3c replayed from the fixture's couples and moves (two populations whose sizes differ after every migration: ids and
    positions part ways): columns 0-2 against the reference's ids before and after each migration, all seven against host.Pedigree"""
    fx = helpers.load_fixture("mig3c")
    n_pop, nchr, nphen, ngen = int(fx["n_pop"]), int(fx["nchr"]), int(fx["nphen"]), int(fx["n_gen"])
    ctx = gpu_lib.create(n_pop, nchr, nphen)
    ctx.set_track_pedigree(True)
    helpers.setup_static(ctx, fx)
    ped = []
    for ip, s in enumerate(helpers.find_gen0_seeds(fx, oracle_lib)):
        ctx.init_gen0(ip, len(fx[f"g0_pop{ip}_sex"]), s)
        ped.append(Pedigree(len(fx[f"g0_pop{ip}_sex"])))
        assert np.array_equal(ctx.download_pedigree(ip), ped_records(ped[ip]))
    for g in range(1, ngen + 1):
        for ip in range(n_pop):
            pre = f"g{g}_pop{ip}_"
            c, ms = fx[pre + "couples"], fx[pre + "mut_seeds"]
            assert np.all(c[:, 2] == 0)
            ctx.reproduce(ip, c, int(fx[pre + "seed_reproduce"]), ms if len(ms) else None)
            ped[ip] = ped[ip].offspring(np.repeat(c[:, 0], c[:, 3]), np.repeat(c[:, 1], c[:, 3]))
            got = ctx.download_pedigree(ip)
            assert np.array_equal(got[:, :3], fx[pre + "ids"]), f"ids of generation {g} population {ip}"
            assert np.array_equal(got, ped_records(ped[ip]))
        if f"g{g}_moves" in fx:
            moves = helpers.derive_moves(fx, g)
            ctx.migrate(moves)
            old = ped
            ped = []
            for ip in range(n_pop):
                gone = np.zeros(len(old[ip].ID), dtype=bool)
                gone[[pos for sp, pos, dp in moves if sp == ip]] = True
                q = old[ip].take(np.flatnonzero(~gone))
                for sp, pos, dp in moves:
                    if dp == ip:
                        q = q.append(old[sp].take(np.array([pos])))
                ped.append(q)
                got = ctx.download_pedigree(ip)
                assert np.array_equal(got[:, :3], fx[f"g{g}_pop{ip}_postmig_ids"]), f"post-migration ids of generation {g} population {ip}"
                assert np.array_equal(got, ped_records(q))
    ctx.close()


# ---- 2. avoid_inbreeding on the device's own ids -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one_call", "mate_then_reproduce"])
def test_assortative_loop_with_inbreeding_test_on_device_ids(gpu_lib, form):
    """am1 (second spouses, --avoid_inbreeding, Poisson families) from --seed alone on the device's selection values, with pedigree ==
    NULL in every mating call: the reference's couples, inbred flags included, and its ids"""
    fx = helpers.load_fixture("am1")
    nchr, nphen, ngen = int(fx["nchr"]), int(fx["nphen"]), int(fx["n_gen"])
    ctx = gpu_lib.create(1, nchr, nphen)
    helpers.setup_static(ctx, fx)
    var = [[float(v) for v in fx[f"pop0_ph{p}_var"]] for p in range(nphen)]
    vc = [float(fx[f"pop0_ph{p}_vc"]) if f"pop0_ph{p}_vc" in fx else 0.0 for p in range(nphen)]
    omega = [float(fx[f"pop0_ph{p}_omega"]) if f"pop0_ph{p}_omega" in fx else 1.0 for p in range(nphen)]
    lam = [float(fx[f"pop0_ph{p}_lambda"]) if f"pop0_ph{p}_lambda" in fx else 1.0 for p in range(nphen)]
    extra = [str(x) for x in fx["args_extra"]]
    assert "--avoid_inbreeding" in extra and ("--vt_type" not in extra or extra[extra.index("--vt_type") + 1] == "1")
    mm = float(extra[extra.index("--MM") + 1]) if "--MM" in extra else 0.0
    sim = Simulation(ctx, int(fx["seed"]), nchr, bool(int(fx["pop0_has_mut"])), track_pedigree=True, device_pedigree=True)
    beta = [1.0] * nphen

    def scale(g, s2, prev, common):
        n = len(sim.sex[0]); outs = []
        for p in range(nphen):
            va, vd, ve, vf = var[p]
            seed = int(sim.ras_glob_seed()[0])
            ff, fm = (host.parental_inputs(prev[p], ctx.download_pedigree(0)).T if g > 0 else np.zeros((2, n)))
            o = ctx.scale_ad_compute_gef(0, p, g, seed, va, vd, ve, vf, beta[p], s2[p][0], s2[p][1], common_sibling=common[p], f_father=ff, f_mother=fm)
            if g > 0:
                close(o["phen"], fx[f"g{g}_pop0_ph{p}_gef_out"][:, 5], f"am1: phenotype {p} generation {g}")
            outs.append(o)
        return outs

    sim.ras_initial_human_gen0(0, len(fx["g0_pop0_sex"]))
    n0 = len(sim.sex[0])
    common0 = [NormalEngine(int(sim.ras_glob_seed()[0])).draw(n0, float(np.sqrt(vc[p]))) if vc[p] > 0 else np.zeros(n0) for p in range(nphen)]
    add, dom, _, _ = ctx.compute_ad(0)
    s2 = [(comm_var(add[:, p]), comm_var(dom[:, p])) for p in range(nphen)]
    outs = scale(0, s2, None, common0)
    ctx.compute_selection(0, 0, "none", 0, 0, omega, lam, want=())
    for p in range(nphen):
        beta[p] = float(np.sqrt(var[p][3] / (2 * comm_var(outs[p]["phen"]))))
    n_inbred = 0
    for g in range(1, ngen + 1):
        pop_size, mat_cor, dist, func, p1, p2 = str(fx["pop0_popinfo"][g - 1]).split()
        prev = [o["phen"] for o in outs]
        if form == "one_call":
            sim.next_generation_am_selected(0, int(pop_size), float(mat_cor), mm, True, dist, want_couples=True)
        else:
            sim.assort_mate_device(0, None, None, int(pop_size), float(mat_cor), mm, True, dist, selected=True)
        c, want = sim.couples[0], fx[f"g{g}_pop0_couples"]
        assert len(c) == len(want) and all(np.array_equal(c[k].astype(np.int64), want[:, j]) for j, k in enumerate(("pos_male", "pos_female", "inbreed", "num_offspring"))), f"couples of generation {g}"
        n_inbred += int(want[:, 2].sum())
        if form != "one_call":
            sim.reproduce(0, g)
        got = ctx.download_pedigree(0)
        assert np.array_equal(got[:, :3], fx[f"g{g}_pop0_ids"]), f"ids of generation {g}"
        assert np.array_equal(got, ped_records(sim.ped[0]))
        n = len(sim.sex[0])
        common = sim.common_sibling(0, vc) if any(v > 0 for v in vc) else [np.zeros(n)] * nphen
        outs = scale(g, s2, prev, common)
        ctx.compute_selection(0, g, func, float(p1), float(p2), omega, lam, want=())
    assert n_inbred > 0, "the fixture has no inbred couple: the test shows nothing"
    ctx.close()


# ---- 3. at size against the host mirror --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 100_000])
def test_device_pedigree_at_size_assortative_and_random(gpu_lib, n):
    """5 generations, assortative with avoid_inbreeding (odd) and random mating (even): all seven ids against host.Pedigree, and the
    couples of gev_assort_mate on the device's ids against the same call on the host mirror's ids (n = 3000: a population in which
    siblings and cousins do meet)"""
    cfg = SyntheticConfig(n, 2048, chrom_bp=4_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=100, seed=5)
    ctx = gpu_lib.create(1, 1, 1)
    ctx.set_track_pedigree(True)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 21)
    ctx.synth_cv_founders(0, 0, 0, 2 * n, 22)
    sim = Simulation(ctx, 777, 1, True, track_pedigree=True)
    sim.device_pedigree = True
    sim.ras_initial_human_gen0(0, n)
    rs = np.random.default_rng(n)
    n_inbred = 0
    for g in range(1, 6):
        n_h = len(sim.sex[0])
        if g % 2:
            mv = rs.standard_normal(n_h)
            seeds = [int(x) for x in sim.ras_glob_seed(4)]
            P = sim.ped[0]
            ped5 = np.stack([P.ID_Father, P.ID_Fathers_Father, P.ID_Fathers_Mother, P.ID_Mothers_Father, P.ID_Mothers_Mother], axis=1)
            want, rw = ctx.assort_mate(0, seeds, mv, None, n, 0.4, 0.1, True, "p", pedigree=ped5)
            c, r = ctx.assort_mate(0, seeds, mv, None, n, 0.4, 0.1, True, "p", pedigree=None)
            assert r == rw and np.array_equal(c, want), f"generation {g}: couples on the device's ids differ from the couples on the host's"
            n_inbred += r["n_inbreed"]
            sim.couples[0] = c
            sim._device_couples = (0, r["n_offspring"])
            sim.reproduce(0, g)
        else:
            sim.next_generation_rm(0, n, None, want_couples=True)
        assert np.array_equal(ctx.download_pedigree(0), ped_records(sim.ped[0])), f"generation {g}"
    if n <= 3_000:
        assert n_inbred > 0
    ctx.close()


# ---- 4. rows removed and imported: dropped, restored, and carried on from physical rows --------------------------------------------
def test_pedigree_dropped_with_the_rows_and_restored_by_upload(gpu_lib):
    n = 400
    cfg = SyntheticConfig(n, 1024, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=50, seed=9)
    ctx = gpu_lib.create(2, 1, 1)
    ctx.set_track_pedigree(True)
    for ip in range(2):
        cfg.apply_static(ctx, ip)
        ctx.synth_founders(ip, 0, 2 * n, 31 + ip)
        ctx.synth_cv_founders(ip, 0, 0, 2 * n, 41 + ip)
    sim = Simulation(ctx, 99, 1, True, track_pedigree=True)
    for ip in range(2):
        sim.ras_initial_human_gen0(ip, n)
    for g in (1, 2):
        for ip in range(2):
            sim.next_generation_rm(ip, n, None, want_couples=True)
    # 30 individuals of population 0 travel to population 1 as packed records; 25 of population 1 are removed
    who = np.arange(5, 65, 2, dtype=np.uint64)
    gone = np.arange(100, 125, dtype=np.uint64)
    nb = ctx.export_size(0, who)
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; hip.hipFree.argtypes = [C.c_void_p]
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), max(nb, 16)) == 0 and buf.value
    try:
        ctx.export_rows(0, who, buf.value, nb)
        ctx.remove_rows(1, gone)
        with pytest.raises(capi.GevError) as e:
            ctx.download_pedigree(1)
        assert e.value.code == -2
        ctx.import_rows(1, buf.value, nb, len(who))
    finally:
        hip.hipFree(buf)
    with pytest.raises(capi.GevError) as e:
        ctx.download_pedigree(1)
    assert e.value.code == -2
    with pytest.raises(capi.GevError) as e:           # the inbreeding test has no ids to read
        ctx.assort_mate(1, [1, 2, 3, 4], np.zeros(ctx.pop_size(1)), None, n, 0.3, 0.0, True, "p", pedigree=None)
    assert e.value.code == -2
    assert np.array_equal(ctx.download_pedigree(0), ped_records(sim.ped[0])), "population 0 was only read"
    keep = np.setdiff1d(np.arange(n), gone.astype(np.int64))
    sim.ped[1] = sim.ped[1].take(keep).append(sim.ped[0].take(who.astype(np.int64)))
    ctx.upload_pedigree(1, ped_records(sim.ped[1]))
    assert np.array_equal(ctx.download_pedigree(1), ped_records(sim.ped[1])), "ids uploaded by position while the positions are not rows"
    # the next generation breeds from rows in their pending order: the parents' ids are found by physical row
    n1 = ctx.pop_size(1)
    assert n1 == n - len(gone) + len(who)
    rs = np.random.default_rng(4)
    c = host.couples_array(rs.integers(0, n1, n), rs.integers(0, n1, n))
    seeds = sim.ras_glob_seed(1 + n)
    ctx.reproduce(1, c, int(seeds[0]), seeds[1:])
    sim.ped[1] = sim.ped[1].offspring(c["pos_male"].astype(np.int64), c["pos_female"].astype(np.int64))
    assert np.array_equal(ctx.download_pedigree(1), ped_records(sim.ped[1]))
    # a pending order that is materialised (gev_migrate does it first) takes the ids along
    ctx.remove_rows(1, np.array([0, 7], dtype=np.uint64))
    sim.ped[1] = sim.ped[1].take(np.setdiff1d(np.arange(n), [0, 7]))
    ctx.upload_pedigree(1, ped_records(sim.ped[1]))
    ctx.migrate([(0, 3, 1), (1, 10, 0)])
    p0, p1 = sim.ped[0], sim.ped[1]
    sim.ped[0] = p0.take(np.setdiff1d(np.arange(n), [3])).append(p1.take(np.array([10])))
    sim.ped[1] = p1.take(np.setdiff1d(np.arange(n - 2), [10])).append(p0.take(np.array([3])))
    for ip in range(2):
        assert np.array_equal(ctx.download_pedigree(ip), ped_records(sim.ped[ip])), f"population {ip} after the migration"
    ctx.close()


# ---- 5. refusals, and nothing changes with tracking off ------------------------------------------------------------------------------
def test_pedigree_refusals(gpu_lib):
    n = 200
    cfg = SyntheticConfig(n, 1024, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=50, seed=2)

    def population(track):
        ctx = gpu_lib.create(1, 1, 1)
        if track:
            ctx.set_track_pedigree(True)
        cfg.apply_static(ctx)
        ctx.synth_founders(0, 0, 2 * n, 3); ctx.synth_cv_founders(0, 0, 0, 2 * n, 4)
        return ctx

    def code(call):
        with pytest.raises(capi.GevError) as e:
            call()
        return e.value.code

    off = population(False)
    assert code(lambda: off.download_pedigree(0)) == -2           # (tracking off comes first: nothing else is looked at)
    off.init_gen0(0, n, 5)
    assert code(lambda: off.download_pedigree(0)) == -2
    assert code(lambda: off.upload_pedigree(0, np.zeros((n, 7), dtype=np.int64))) == -2
    assert code(lambda: off.set_track_pedigree(True)) == -2, "tracking cannot start behind gev_init_gen0"
    mv = np.linspace(-1, 1, n)
    assert code(lambda: off.assort_mate(0, [1, 2, 3, 4], mv, None, n, 0.3, 0.0, True, "p", pedigree=None)) == -1, "avoid_inbreeding + NULL pedigree without tracking stays GEV_EINVAL"
    assert code(lambda: off.generation_begin_assort(0, 12345, n, 0.3, 0.0, True, "p", mating_value=mv, pedigree=None)) == -1
    ped5 = np.tile(np.arange(n, dtype=np.int64)[:, None], (1, 5))
    c_off, r_off = off.assort_mate(0, [1, 2, 3, 4], mv, None, n, 0.3, 0.0, True, "p", pedigree=ped5)
    on = population(True)
    assert code(lambda: on.download_pedigree(0)) == -2            # no current generation
    on.init_gen0(0, n, 5)
    assert np.array_equal(on.download_pedigree(0), np.tile(np.arange(n, dtype=np.int64)[:, None], (1, 7))), "generation 0: every id = i"
    c_on, r_on = on.assort_mate(0, [1, 2, 3, 4], mv, None, n, 0.3, 0.0, True, "p", pedigree=None)
    assert r_on == r_off and np.array_equal(c_on, c_off), "generation 0 on the device's ids = the host's identity ids"
    c_h, r_h = on.assort_mate(0, [1, 2, 3, 4], mv, None, n, 0.3, 0.0, True, "p", pedigree=ped5)
    assert r_h == r_off and np.array_equal(c_h, c_off), "a pedigree the host passes is still the one that is used"
    with pytest.raises(ValueError):
        on.upload_pedigree(0, np.zeros((n - 1, 7), dtype=np.int64))
    off.close(); on.close()


# =====================================================================================================================================
# gev_generation_phenotypes: ras_scale_AD_compute_GEF of every phenotype from the library's own state
# =====================================================================================================================================
def loop_close(a, b, what):
    """floats carried through a closed loop (tests/helpers.py:close)"""
    assert np.allclose(a, b, rtol=1e-9, atol=1e-12), f"{what}: max abs diff {np.max(np.abs(np.asarray(a) - np.asarray(b)))}"


def check_var(ctx, r, nphen, what):
    """var[p][7] against CommFunc::var of the downloaded components: 1e-12, exactly 0 where a component is all zero"""
    comps = [ctx.download_phenotypes(0, p) for p in range(nphen)]
    for p in range(nphen):
        for j, name in enumerate(capi.PHENOTYPE_COMPONENTS):
            v = comps[p][name]
            if not np.any(v):
                assert r["var"][p][j] == 0.0, f"{what}: var of the all-zero {name} of phenotype {p}"
            else:
                want = comm_var(v)
                assert abs(r["var"][p][j] - want) <= 1e-12 * abs(want), f"{what}: var({name}) of phenotype {p}: {r['var'][p][j]!r} vs {want!r}"
    return comps


def adjusted_beta(var7, vf, vt_type):
    """"adjust beta" behind generation 0 (:648-657) from var alone: on var(P), or (vt_type 2) on var(F) when that is > 0"""
    if not vf > 0:
        return 1.0
    if vt_type == 1:
        return float(np.sqrt(vf / (2 * var7[6])))
    if vt_type == 2 and var7[5] > 0:
        return float(np.sqrt(vf / (2 * var7[5])))
    return 1.0


def device_phenotype_loop(gpu_lib, case, chain=False, short_candidates=False, check=True):
    """Simulation::run of a single-population fixture from --seed alone with NO per-individual array uploaded after generation 0:
    mating on the device's selection values, whole generations in one call pair, phenotypes by gev_generation_phenotypes, the saved
    record by gev_save_prev_gen.  -> what the run computed (couples, sexes, components per generation)"""
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
    mm = float(extra[extra.index("--MM") + 1]) if "--MM" in extra else 0.0
    avoid = "--avoid_inbreeding" in extra
    sim = Simulation(ctx, int(fx["seed"]), nchr, bool(int(fx["pop0_has_mut"])), device_pedigree=True)
    if short_candidates:
        ctx.dbg_phenotype_knobs(True)
    if chain:
        ctx.set_generation_chain(nphen)
    beta = [1.0] * nphen
    schemes = lambda: [(var[p][0], var[p][1], vc[p], var[p][2], var[p][3], beta[p]) for p in range(nphen)]
    rec = {"couples": [], "sex": [], "comps": [], "var": [], "seeds": []}
    sim.ras_initial_human_gen0(0, len(fx["g0_pop0_sex"]))
    assert np.array_equal(sim.sex[0], fx["g0_pop0_sex"])
    sim.generation_phenotypes(0, 0, schemes(), vt_type)
    r = sim.phenotypes_result(0)
    assert len(r["seeds"]) == nphen + sum(v > 0 for v in vc)
    comps = check_var(ctx, r, nphen, f"{case} generation 0")
    rec["comps"].append(comps); rec["var"].append(r["var"]); rec["seeds"].append(r["seeds"])
    for p in range(nphen):
        va0, vd0 = ctx.get_ad_gen0(0, p)
        add, dom, _, _ = ctx.compute_ad(0, per_chr=False)
        assert abs(va0 - comm_var(add[:, p])) <= 1e-12 * abs(va0) and abs(vd0 - comm_var(dom[:, p])) <= 1e-12 * abs(vd0) + 0.0
        beta[p] = adjusted_beta(r["var"][p], var[p][3], vt_type)
    ctx.compute_selection(0, 0, "none", 0, 0, omega, lam, want=())
    sim.save_prev_gen(0)
    for g in range(1, ngen + 1):
        pop_size, mat_cor, dist, func, p1, p2 = str(fx["pop0_popinfo"][g - 1]).split()
        if rm:
            res = sim.next_generation_rm_selected(0, int(pop_size), want_couples=True)
            assert int(res["seed_mate"]) == int(fx[f"g{g}_pop0_mate_seed"])
        else:
            res = sim.next_generation_am_selected(0, int(pop_size), float(mat_cor), mm, avoid, dist, want_couples=True)
        c, want = sim.couples[0], fx[f"g{g}_pop0_couples"]
        if check:
            assert len(c) == len(want) and all(np.array_equal(c[k].astype(np.int64), want[:, j]) for j, k in enumerate(("pos_male", "pos_female", "inbreed", "num_offspring"))), f"{case}: couples of generation {g}"
            assert int(res["seed_reproduce"]) == int(fx[f"g{g}_pop0_seed_reproduce"]) and np.array_equal(sim.sex[0], fx[f"g{g}_pop0_sex"]), f"{case}: generation {g}"
            assert np.array_equal(ctx.download_pedigree(0)[:, :3], fx[f"g{g}_pop0_ids"])
        sim.generation_phenotypes(0, g, schemes(), vt_type)
        ctx.compute_selection(0, g, func, float(p1), float(p2), omega, lam, want=())       # enqueued behind it: nothing waited for in between
        r = sim.phenotypes_result(0)
        if short_candidates:                     # (the step was run again: the selection values are computed from the second run)
            ctx.compute_selection(0, g, func, float(p1), float(p2), omega, lam, want=())
        comps = check_var(ctx, r, nphen, f"{case} generation {g}")
        if check:
            assert np.array_equal(r["seeds"], [int(fx[f"g{g}_pop0_ph{p}_gef_seed"]) for p in range(nphen)]), f"{case}: seeds of generation {g}"
            for p in range(nphen):
                gi, go = fx[f"g{g}_pop0_ph{p}_gef_in"], fx[f"g{g}_pop0_ph{p}_gef_out"]
                close(comps[p]["common_sibling"], gi[:, 0], f"{case}: C of phenotype {p} generation {g}")
                for j, name in enumerate(helpers.GEF_OUTPUTS):
                    loop_close(comps[p][name], go[:, j], f"{case}: {name} of phenotype {p} generation {g}")
        sim.save_prev_gen(0)
        rec["couples"].append(c.copy()); rec["sex"].append(sim.sex[0].copy()); rec["comps"].append(comps); rec["var"].append(r["var"]); rec["seeds"].append(r["seeds"])
    rec["reruns"] = ctx.dbg_phenotype_knobs(False)
    rec["chain"] = chain
    ctx.close()
    return rec


@pytest.mark.parametrize("case", ["vc1", "vt2", "dense", "om1", "sel1", "am1"])
def test_closed_loop_with_device_phenotypes(gpu_lib, case):
    """couples, sexes, seeds, ids exact; the family effect within 1e-12 of the reference's recorded one; the six outputs within the
    closed-loop tolerance; var[p][7] against comm_var of the downloaded components; beta adjusted from var alone"""
    rec = device_phenotype_loop(gpu_lib, case)
    assert rec["reruns"] == 0


def same_run(a, b):
    for x, y in zip(a["couples"], b["couples"]):
        assert np.array_equal(x, y)
    for x, y in zip(a["sex"], b["sex"]):
        assert np.array_equal(x, y)
    for x, y in zip(a["seeds"], b["seeds"]):
        assert np.array_equal(x, y)
    for ga, gb in zip(a["comps"], b["comps"]):
        for pa, pb in zip(ga, gb):
            for name in capi.PHENOTYPE_COMPONENTS:
                assert helpers.bits_equal(pa[name], pb[name]), name
    for x, y in zip(a["var"], b["var"]):
        assert helpers.bits_equal(x, y)


@pytest.mark.parametrize("case", ["dense", "vt2"])
def test_head_start_with_device_phenotypes(gpu_lib, case):
    """gev_set_generation_chain(nphen): the phenotype step makes exactly the draws the host promised, and the run is the same run"""
    same_run(device_phenotype_loop(gpu_lib, case, chain=True), device_phenotype_loop(gpu_lib, case))


@pytest.mark.parametrize("case", ["vc1", "dense"])
def test_short_candidate_streams_are_run_again(gpu_lib, case):
    """the test hook starts every normal stream with too few candidate pairs: gev_phenotypes_result runs the step again, same values"""
    short = device_phenotype_loop(gpu_lib, case, short_candidates=True)
    assert short["reruns"] > 0
    same_run(short, device_phenotype_loop(gpu_lib, case))


# ---- one step against the reference's recorded inputs ------------------------------------------------------------------------------
def glob_state_in_front_of(fx, seeds):
    """glob_generator's state in front of the draws that gave `seeds` in the reference's run (found in its ras_glob_seed() stream)"""
    from geneevolve_amd.host import GlobSeedStream
    seeds = np.asarray(seeds, dtype=np.uint32)
    vals = GlobSeedStream(int(fx["seed"])).draw(400_000)
    hit = np.flatnonzero(vals[:len(vals) - len(seeds)] == seeds[0])
    hit = [i for i in hit if np.array_equal(vals[i:i + len(seeds)], seeds)]
    assert len(hit) >= 1, "the recorded seeds are not in the stream"
    st = GlobSeedStream(int(fx["seed"]))
    st.draw(int(hit[0]))
    return st.x


def recorded_step(ctx, fx, g, ip, nphen, prev_of, label, expect_range_error=False):
    """gev_generation_phenotypes of population ip at generation g from the recorded generation-0 variances, saved record and seeds"""
    pars = [[float(x) for x in fx[f"g{g}_pop{ip}_ph{p}_gef_par"]] for p in range(nphen)]          # s2a, s2d, va, vd, ve, vf, beta
    vc = [float(fx[f"pop{ip}_ph{p}_vc"]) if f"pop{ip}_ph{p}_vc" in fx else 0.0 for p in range(nphen)]
    vt = int(fx[f"g{g}_pop{ip}_ph0_gef_vt"])
    for p in range(nphen):
        ctx.set_ad_gen0(ip, p, pars[p][0], pars[p][1])
    ctx.upload_prev_gen(ip, np.stack([prev_of(p, 5) for p in range(nphen)]), np.stack([prev_of(p, 4) for p in range(nphen)]))
    seeds = [int(fx[f"g{g}_pop{ip}_ph{p}_gef_seed"]) for p in range(nphen)]
    ctx.generation_phenotypes(ip, g, glob_state_in_front_of(fx, seeds), [(q[2], q[3], vc[p], q[4], q[5], q[6]) for p, q in enumerate(pars)], vt)
    if expect_range_error:
        with pytest.raises(capi.GevError) as e:
            ctx.phenotypes_result(ip)
        assert e.value.code == -5, str(e.value)
        return
    r = ctx.phenotypes_result(ip)
    assert np.array_equal(r["seeds"], seeds), f"{label}: seeds"
    for p in range(nphen):
        got = ctx.download_phenotypes(ip, p)
        gi, want = fx[f"g{g}_pop{ip}_ph{p}_gef_in"], fx[f"g{g}_pop{ip}_ph{p}_gef_out"]
        close(got["common_sibling"], gi[:, 0], f"{label}: C of phenotype {p}")
        helpers.check_gef_outputs(got, want, g, pars[p][4], pars[p][5], 1e-12, f"{label} phenotype {p}")


@pytest.mark.parametrize("case", ["vc1", "dense", "vt2"])
def test_one_phenotype_step_against_recorded_inputs(gpu_lib, oracle_lib, case):
    """generations 2... replayed from the fixture's couples: A, D, G and F (the gather by id) bit for bit, C, E and P within 1e-12"""
    fx = helpers.load_fixture(case)
    nchr, nphen, ngen = int(fx["nchr"]), int(fx["nphen"]), int(fx["n_gen"])
    ctx = gpu_lib.create(1, nchr, nphen)
    ctx.set_track_pedigree(True)
    helpers.setup_static(ctx, fx)
    ctx.init_gen0(0, len(fx["g0_pop0_sex"]), helpers.find_gen0_seeds(fx, oracle_lib)[0])
    for g in range(1, ngen + 1):
        ms = fx[f"g{g}_pop0_mut_seeds"]
        ctx.reproduce(0, fx[f"g{g}_pop0_couples"], int(fx[f"g{g}_pop0_seed_reproduce"]), ms if len(ms) else None)
        if g >= 2:
            recorded_step(ctx, fx, g, 0, nphen, lambda p, col: fx[f"g{g - 1}_pop0_ph{p}_gef_out"][:, col], f"{case} generation {g}")
    ctx.close()


def test_phenotype_step_reads_the_saved_record_by_id_after_migration(gpu_lib, oracle_lib):
    """mig3c in one context, couples and moves replayed, ids tracked by the device, the saved record of both populations uploaded
    from the recorded outputs carried through the recorded moves.  Population 0 (ids and positions differ): F bit for bit.
    Population 1: ids run past its saved record (the reference reads past the end of its array): GEV_EUNSUPPORTED, and the context
    stays usable"""
    from tests.test_phenotypes_cpu import saved_record
    fx = helpers.load_fixture("mig3c")
    n_pop, nchr, nphen, ngen = int(fx["n_pop"]), int(fx["nchr"]), int(fx["nphen"]), int(fx["n_gen"])
    ctx = gpu_lib.create(n_pop, nchr, nphen)
    ctx.set_track_pedigree(True)
    helpers.setup_static(ctx, fx)
    for ip, s in enumerate(helpers.find_gen0_seeds(fx, oracle_lib)):
        ctx.init_gen0(ip, len(fx[f"g0_pop{ip}_sex"]), s)
    n_refused = 0
    for g in range(1, ngen + 1):
        for ip in range(n_pop):
            pre = f"g{g}_pop{ip}_"
            ms = fx[pre + "mut_seeds"]
            ctx.reproduce(ip, fx[pre + "couples"], int(fx[pre + "seed_reproduce"]), ms if len(ms) else None)
            if g >= 2:
                ids = fx[pre + "ids"]
                n_prev = len(saved_record(fx, g, 0, 5)[ip])
                beyond = bool(np.any(ids[:, 1:3] >= n_prev))
                assert beyond == (ip == 1)
                recorded_step(ctx, fx, g, ip, nphen, lambda p, col: saved_record(fx, g, p, col)[ip], f"mig3c generation {g} population {ip}", expect_range_error=beyond)
                n_refused += beyond
                if beyond:
                    with pytest.raises(capi.GevError) as e:      # nothing published for the selection step
                        ctx.compute_selection(ip, g, "none", 0, 0, [1.0] * nphen, [1.0] * nphen, want=())
                    assert e.value.code == -2
        ctx.migrate(helpers.derive_moves(fx, g))
        for ip in range(n_pop):
            assert np.array_equal(ctx.download_pedigree(ip)[:, :3], fx[f"g{g}_pop{ip}_postmig_ids"])
    assert n_refused == ngen - 1
    ctx.close()


# ---- at size against the host mirror ------------------------------------------------------------------------------------------------
def sized_run(gpu_lib, n, short_candidates):
    cfg = SyntheticConfig(n, 2048, chrom_bp=4_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=100, nphen=2, seed=6, vd=0.2)
    ctx = gpu_lib.create(1, 1, 2)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 51)
    for p in range(2):
        ctx.synth_cv_founders(0, p, 0, 2 * n, 52 + p)
    sim = Simulation(ctx, 4242, 1, True, track_pedigree=True, device_pedigree=True)
    if short_candidates:
        ctx.dbg_phenotype_knobs(True)
    sim.ras_initial_human_gen0(0, n)
    vt_type = 1
    base = [(0.5, 0.1, 0.1, 0.2, 0.1), (0.4, 0.0, 0.2, 0.3, 0.1)]               # va, vd, vc, ve, vf
    beta = [1.0, 1.0]
    schemes = lambda: [b + (beta[p],) for p, b in enumerate(base)]
    vc = [b[2] for b in base]
    sim.generation_phenotypes(0, 0, schemes(), vt_type)
    r = sim.phenotypes_result(0)
    comps = [ctx.download_phenotypes(0, p) for p in range(2)]
    for p in range(2):                                                          # generation 0: engines of their own seeds (:3053-3066, :3095)
        close(comps[p]["common_sibling"], NormalEngine(int(r["seeds"][p])).draw(n, float(np.sqrt(vc[p]))), f"generation-0 C of phenotype {p}")
        close(comps[p]["parental_effect"], NormalEngine(int(r["seeds"][2 + p]) + 1).draw(n, float(np.sqrt(base[p][4]))), f"generation-0 F of phenotype {p}")
        beta[p] = adjusted_beta(r["var"][p], base[p][4], vt_type)
    ctx.compute_selection(0, 0, "none", 0, 0, [1.0, 0.5], [1.0, 1.0], want=())
    sim.save_prev_gen(0)
    out = [comps]
    for g in range(1, 6):
        prev = [c["phen"] for c in out[-1]]
        if g % 2:
            sim.next_generation_am_selected(0, n, 0.3, 0.1, True, "p", want_couples=True)
        else:
            sim.next_generation_rm_selected(0, n, want_couples=True)
        ids = ctx.download_pedigree(0)
        assert np.array_equal(ids, ped_records(sim.ped[0])), f"ids of generation {g}"
        sim.generation_phenotypes(0, g, schemes(), vt_type)
        ctx.compute_selection(0, g, "logit", 0.2, 0.8, [1.0, 0.5], [1.0, 1.0], want=())
        r = sim.phenotypes_result(0)
        if short_candidates:
            ctx.compute_selection(0, g, "logit", 0.2, 0.8, [1.0, 0.5], [1.0, 1.0], want=())
        comps = check_var(ctx, r, 2, f"generation {g}") if g == 5 or n <= 5000 else [ctx.download_phenotypes(0, p) for p in range(2)]
        common = sim.common_sibling(0, vc)
        for p in range(2):
            close(comps[p]["common_sibling"], common[p], f"C of phenotype {p} generation {g}")
            ff, fm = host.parental_inputs(prev[p], ids).T
            assert helpers.bits_equal(comps[p]["parental_effect"], beta[p] * (ff + fm)), f"F of phenotype {p} generation {g}"
        sim.save_prev_gen(0)
        out.append(comps)
    reruns = ctx.dbg_phenotype_knobs(False)
    ctx.close()
    return out, reruns


@pytest.mark.parametrize("n", [2_000, 100_000])
def test_device_phenotypes_at_size(gpu_lib, n):
    """two phenotypes with vc > 0 and vf > 0, assortative with avoid_inbreeding and random mating, 5 generations: ids, C, F and var
    against the host mirror (Pedigree, common_sibling, parental_inputs, comm_var); the forced rerun gives the same values"""
    a, ra = sized_run(gpu_lib, n, False)
    b, rb = sized_run(gpu_lib, n, True)
    assert ra == 0 and rb >= 6
    for ga, gb in zip(a, b):
        for pa, pb in zip(ga, gb):
            for name in capi.PHENOTYPE_COMPONENTS:
                assert helpers.bits_equal(pa[name], pb[name]), name


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_phenotype_step_refusals(gpu_lib):
    n = 300
    cfg = SyntheticConfig(n, 1024, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=50, seed=2)

    def population(track):
        ctx = gpu_lib.create(1, 1, 1)
        cfg.apply_static(ctx)
        ctx.synth_founders(0, 0, 2 * n, 3); ctx.synth_cv_founders(0, 0, 0, 2 * n, 4)
        sim = Simulation(ctx, 11, 1, True, device_pedigree=track)
        sim.ras_initial_human_gen0(0, n)
        return ctx, sim

    def code(call):
        with pytest.raises(capi.GevError) as e:
            call()
        return e.value.code

    scheme = [(0.5, 0.0, 0.1, 0.3, 0.1, 1.0)]
    off, so = population(False)
    assert code(lambda: so.generation_phenotypes(0, 0, scheme)) == -2, "tracking off"
    assert code(lambda: off.phenotypes_result(0)) == -2
    assert code(lambda: off.download_phenotypes(0, 0)) == -2
    assert code(lambda: off.save_prev_gen(0)) == -2
    off.close()
    ctx, sim = population(True)
    assert code(lambda: sim.generation_phenotypes(0, 1, scheme)) == -2, "generation > 0 without generation-0 variances"
    sim.generation_phenotypes(0, 0, scheme)
    sim.phenotypes_result(0)
    assert code(lambda: ctx.phenotypes_result(0)) == -2, "a result is handed out once"
    ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0], want=())
    sim.next_generation_rm_selected(0, n, want_couples=True)
    assert code(lambda: sim.generation_phenotypes(0, 1, scheme)) == -2, "vf > 0 at generation 1 without a saved record"
    sim.generation_phenotypes(0, 1, [(0.5, 0.0, 0.1, 0.3, 0.0, 1.0)])                  # vf = 0 needs none
    sim.phenotypes_result(0)
    sim.save_prev_gen(0)
    ctx.remove_rows(0, np.array([1, 2], dtype=np.uint64))
    assert code(lambda: sim.generation_phenotypes(0, 1, scheme)) == -2, "the ids were dropped with the rows"
    ids = np.tile(np.arange(n - 2, dtype=np.int64)[:, None], (1, 7))
    ctx.upload_pedigree(0, ids)
    assert code(lambda: sim.generation_phenotypes(0, 1, scheme)) == -2, "the couples' family effects cannot be handed out to other rows"
    sim.generation_phenotypes(0, 1, [(0.5, 0.0, 0.0, 0.3, 0.1, 1.0)])                  # vc = 0: the gather alone, by the uploaded ids
    sim.phenotypes_result(0)
    assert ctx.pop_size(0) == n - 2 and len(ctx.download_phenotypes(0, 0)["phen"]) == n - 2
    ctx.close()


# ---- the device's own record through a migration -------------------------------------------------------------------------------------
def test_saved_record_and_components_follow_a_migration(gpu_lib):
    """two populations, vf > 0 and vc > 0, random mating at constant equal sizes, the same number of migrants each way (every id stays
    below the post-migration size): gev_migrate, then gev_save_prev_gen, 4 generations.  The components arrive with the migrants; the
    next generation's F is beta * (record[ID_Father] + record[ID_Mother]) with the record in post-migration POSITION order and the ids
    the children inherited -- against the host mirror (Pedigree.take / append, parental_inputs)"""
    n, k = 500, 20
    cfg = SyntheticConfig(n, 1024, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=60, seed=8)
    ctx = gpu_lib.create(2, 1, 1)
    for ip in range(2):
        cfg.apply_static(ctx, ip)
        ctx.synth_founders(ip, 0, 2 * n, 61 + ip)
        ctx.synth_cv_founders(ip, 0, 0, 2 * n, 71 + ip)
    sim = Simulation(ctx, 31337, 1, True, track_pedigree=True, device_pedigree=True)
    base = (0.5, 0.0, 0.1, 0.3, 0.1)
    beta = [1.0, 1.0]
    for ip in range(2):
        sim.ras_initial_human_gen0(ip, n)
    for ip in range(2):
        sim.generation_phenotypes(ip, 0, [base + (1.0,)])
        r = sim.phenotypes_result(ip)
        beta[ip] = adjusted_beta(r["var"][0], base[4], 1)
        ctx.compute_selection(ip, 0, "none", 0, 0, [1.0], [1.0], want=())
        sim.save_prev_gen(ip)
    record = [ctx.download_phenotypes(ip, 0)["phen"] for ip in range(2)]
    rs = np.random.default_rng(12)
    n_moved_ids = 0
    for g in range(1, 5):
        comps = []
        for ip in range(2):
            sim.next_generation_rm_selected(ip, n, want_couples=True)
            ids = ctx.download_pedigree(ip)
            assert np.array_equal(ids, ped_records(sim.ped[ip])), f"ids of generation {g} population {ip}"
            n_moved_ids += int(np.sum(ids[:, 1] != sim.couples[ip]["pos_male"].astype(np.int64)))
            sim.generation_phenotypes(ip, g, [base + (beta[ip],)])
            sim.phenotypes_result(ip)
            c = ctx.download_phenotypes(ip, 0)
            ff, fm = host.parental_inputs(record[ip], ids).T
            assert helpers.bits_equal(c["parental_effect"], beta[ip] * (ff + fm)), f"F of generation {g} population {ip}"
            close(c["common_sibling"], sim.common_sibling(ip, [base[2]])[0], f"C of generation {g} population {ip}")
            loop_close(c["phen"], c["additive"] + c["dominance"] + c["common_sibling"] + c["e_noise"] + c["parental_effect"], f"P of generation {g} population {ip}")
            ctx.compute_selection(ip, g, "logit", 0.0, 1.0, [1.0], [1.0], want=())
            comps.append(c)
        moves = [(0, int(p), 1) for p in sorted(rs.choice(n, k, replace=False), reverse=True)] + [(1, int(p), 0) for p in sorted(rs.choice(n, k, replace=False), reverse=True)]
        sim.ras_do_migration(moves)
        old_ped = [sim.ped[0], sim.ped[1]]
        for ip in range(2):
            gone = np.zeros(n, dtype=bool)
            gone[[pos for sp, pos, dp in moves if sp == ip]] = True
            keep = np.flatnonzero(~gone)
            came = np.array([pos for sp, pos, dp in moves if dp == ip])
            sim.ped[ip] = old_ped[ip].take(keep).append(old_ped[1 - ip].take(came))
            sim.sex[ip] = None
            assert np.array_equal(ctx.download_pedigree(ip), ped_records(sim.ped[ip])), f"post-migration ids of generation {g} population {ip}"
            got = ctx.download_phenotypes(ip, 0)
            for name in capi.PHENOTYPE_COMPONENTS:
                assert helpers.bits_equal(got[name], np.concatenate([comps[ip][name][keep], comps[1 - ip][name][came]])), f"{name} behind the migration of generation {g}"
            sim.save_prev_gen(ip)
            record[ip] = got["phen"]
    assert n_moved_ids > 0, "ids never differed from positions: the test shows nothing"
    ctx.close()
