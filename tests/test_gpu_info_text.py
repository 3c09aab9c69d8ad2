"""gev_format_info_text: Population::ras_save_human_info's file (reference src/Population.cpp:510-568) written on the device, byte for
byte -- the device %g against the same header built for the host, closed loops against the host formatter (host.ras_save_human_info)
of the downloaded arrays and against the reference's recorded files, at a size that makes the offset scan loop, behind a migration,
and the refusals."""
import hashlib

import numpy as np
import pytest

from geneevolve_amd import capi, host
from geneevolve_amd.host import Simulation, SyntheticConfig
from tests import helpers
from tests import info_text_inputs as I
from tests.test_gpu_phenotypes import adjusted_beta

pytestmark = pytest.mark.gpu


# ---- %g on the device ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g_ctx(gpu_lib):
    ctx = gpu_lib.create(1, 1, 1)
    yield ctx
    ctx.close()


def g_inputs():
    edges = np.array(I.EDGES + [-v for v in I.EDGES])
    return np.concatenate([edges, I.random_patterns(), I.near_midpoints(), I.normals()])


def test_device_g_equals_the_host_build(gpu_lib, g_ctx):
    x = g_inputs()
    want, want_exact = gpu_lib.dbg_format_g_host(x)
    got, got_exact = g_ctx.dbg_format_g(x)
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert len(bad) == 0, f"{len(bad)} of {len(x)} values differ, first: {[(x[i], bytes(got[i]), bytes(want[i])) for i in bad[:3]]}"
    assert got_exact == want_exact and got_exact > 0
    ne = len(I.EDGES) * 2
    assert I.strings(got[:ne]) == [I.glibc_g(float(v)) for v in x[:ne]]          # and the edge list against the C library itself


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 65537])
def test_device_g_sizes(gpu_lib, g_ctx, n):
    """a partial wave, a full one, more than one block, more than 256 blocks; the tail of the set holds the near-midpoint values"""
    x = g_inputs()
    x = np.concatenate([x[:n // 2], x[len(x) - (n - n // 2):]]) if n > 1 else x[7:8]
    want, want_exact = gpu_lib.dbg_format_g_host(x)
    got, got_exact = g_ctx.dbg_format_g(x)
    assert np.array_equal(got, want) and got_exact == want_exact


# ---- the file ----------------------------------------------------------------------------------------------------------------------------
def host_text(ctx, ipop, sex, nphen):
    """the host formatter on what the downloads return (NaNs, if any, through the C library: Python prints no sign for them)"""
    ids = ctx.download_pedigree(ipop)
    ped = host.Pedigree(len(ids))
    for j, f in enumerate(("ID", "ID_Father", "ID_Mother", "ID_Fathers_Father", "ID_Fathers_Mother", "ID_Mothers_Father", "ID_Mothers_Mother")):
        setattr(ped, f, ids[:, j].copy())
    comps = [ctx.download_phenotypes(ipop, p) for p in range(nphen)]
    sel = ctx.download_selection(ipop)
    arrays = [c[k] for c in comps for k in capi.PHENOTYPE_COMPONENTS] + list(sel.values())
    if any(np.isnan(a).any() for a in arrays):
        cols = np.stack(arrays, axis=1)
        hdr = host.ras_save_human_info(ped.take(np.arange(0)), sex[:0], [{k: c[k][:0] for k in capi.PHENOTYPE_COMPONENTS} for c in comps], *[v[:0] for v in sel.values()])
        rows = [b" ".join([b"%d" % (v + 1) for v in ids[i]] + [b"%d" % sex[i]] + [I.glibc_g(float(v)) for v in cols[i]]) + b"\n" for i in range(len(ids))]
        return hdr + b"".join(rows)
    return host.ras_save_human_info(ped, sex, comps, sel["mating_value"], sel["selection_value"], sel["selection_value_func"])


def check_text(ctx, ipop, sex, nphen, what, slices=True):
    want = host_text(ctx, ipop, sex, nphen)
    got = ctx.format_info_text(ipop)
    if got != want:
        la, lb = got.split(b"\n"), want.split(b"\n")
        first = next((i for i, (a, b) in enumerate(zip(la, lb)) if a != b), min(len(la), len(lb)))
        raise AssertionError(f"{what}: {len(got)} bytes vs {len(want)}; first differing line {first}: {la[first:first + 1]} vs {lb[first:first + 1]}")
    assert ctx.info_text_size(ipop) == len(want), f"{what}: size query"
    if slices:
        n = ctx.pop_size(ipop)
        hdr = ctx.format_info_text(ipop, 0, 0)
        assert hdr == want[:want.index(b"\n") + 1] and ctx.format_info_text(ipop, 0, 0, header=False) == b""
        parts = [ctx.format_info_text(ipop, a, b - a, header=False) for a, b in ((0, 1), (1, n - 1), (n - 1, n))]
        assert hdr + b"".join(parts) == want, f"{what}: slices"
        nb = capi.C.c_size_t()
        buf = np.zeros(len(want), dtype=np.uint8)
        rc = ctx.L._f("format_info_text")(ctx.h, ipop, 0, n, 1, buf, len(want) - 1, capi.C.byref(nb))
        assert rc == -1 and nb.value == len(want), f"{what}: one byte too few"
        rc = ctx.L._f("format_info_text")(ctx.h, ipop, 0, n, 1, buf, len(want), capi.C.byref(nb))
        assert rc == 0 and buf.tobytes() == want, f"{what}: a buffer of exactly the size"
    return got


def info_loop(gpu_lib, case):
    """tests/test_gpu_phenotypes.py:device_phenotype_loop with the text taken after every generation's selection values"""
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
    beta = [1.0] * nphen
    schemes = lambda: [(var[p][0], var[p][1], vc[p], var[p][2], var[p][3], beta[p]) for p in range(nphen)]
    texts = []
    sim.ras_initial_human_gen0(0, len(fx["g0_pop0_sex"]))
    sim.generation_phenotypes(0, 0, schemes(), vt_type)
    r = sim.phenotypes_result(0)
    for p in range(nphen):
        beta[p] = adjusted_beta(r["var"][p], var[p][3], vt_type)
    ctx.compute_selection(0, 0, "none", 0, 0, omega, lam, want=())
    texts.append(check_text(ctx, 0, sim.sex[0], nphen, f"{case} generation 0"))
    sim.save_prev_gen(0)
    for g in range(1, ngen + 1):
        pop_size, mat_cor, dist, func, p1, p2 = str(fx["pop0_popinfo"][g - 1]).split()
        if rm:
            sim.next_generation_rm_selected(0, int(pop_size), want_couples=True)
        else:
            sim.next_generation_am_selected(0, int(pop_size), float(mat_cor), mm, avoid, dist, want_couples=True)
        assert np.array_equal(sim.sex[0], fx[f"g{g}_pop0_sex"]), f"{case}: generation {g}"
        sim.generation_phenotypes(0, g, schemes(), vt_type)
        ctx.compute_selection(0, g, func, float(p1), float(p2), omega, lam, want=())
        sim.phenotypes_result(0)
        texts.append(check_text(ctx, 0, sim.sex[0], nphen, f"{case} generation {g}"))
        assert sim.save_human_info(0) == texts[-1]
        sim.save_prev_gen(0)
    ctx.close()
    return fx, texts


LOOP_CASES = ["vc1", "vt2", "am1", "sel1", "om1"]
_loops = {}


def loop_of(gpu_lib, case):
    if case not in _loops:
        _loops[case] = info_loop(gpu_lib, case)
    return _loops[case]


@pytest.mark.parametrize("case", LOOP_CASES)
def test_closed_loop_text_equals_the_host_formatter(gpu_lib, case):
    fx, texts = loop_of(gpu_lib, case)
    assert len(texts) == int(fx["n_gen"]) + 1


@pytest.mark.parametrize("case", LOOP_CASES)
def test_closed_loop_text_against_the_reference(gpu_lib, oracle_lib, case):
    """SHA-256 against the reference's recorded files (reported: device floats agree to 1e-12, not bit for bit), and field by field
    against the exact oracle build's texts with the bounds of test_info_files_with_device_phenotype_scaling"""
    fx, texts = loop_of(gpu_lib, case)
    have = [g for g in range(len(texts)) if f"infofile_pop0_gen{g}_sha" in fx]
    match = sum(np.array_equal(np.frombuffer(hashlib.sha256(texts[g]).digest(), dtype=np.uint8), fx[f"infofile_pop0_gen{g}_sha"]) for g in have)
    print(f"{case}: {match} of {len(have)} device-written .info files equal the reference's byte for byte")
    t_ref = []
    helpers.closed_loop_case(oracle_lib, fx, f"oracle/{case}", exact=True, info_texts=t_ref)
    assert len(t_ref) == len(texts)
    total = differing = 0
    for g, (a, b) in enumerate(zip(texts, t_ref)):
        la, lb = a.decode().splitlines(), b.decode().splitlines()
        assert len(la) == len(lb) and la[0] == lb[0], f"{case} generation {g}: header / number of rows"
        for x, y in zip(la[1:], lb[1:]):
            fa, fb = x.split(), y.split()
            assert len(fa) == len(fb) and fa[:8] == fb[:8], f"{case} generation {g}: ids and sex are exact"
            total += len(fa)
            for u, v in zip(fa[8:], fb[8:]):
                if u != v:
                    differing += 1
                    assert abs(float(u) - float(v)) <= 2e-6 * max(abs(float(v)), 1e-300) + 1e-12, f"{case}: field {u} vs {v}"
    print(f"{case}: {differing} of {total} text fields differ from the exact build's (last printed digit)")
    assert differing <= total * 1e-3


def test_text_at_a_size_that_makes_the_offset_scan_loop(gpu_lib):
    """65 537 individuals = 1025 blocks of rows: the scan of the block sums takes more than one round of 256"""
    n = 65537
    cfg = SyntheticConfig(n, 2048, chrom_bp=4_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=100, nphen=2, seed=6, vd=0.2)
    ctx = gpu_lib.create(1, 1, 2)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 51)
    for p in range(2):
        ctx.synth_cv_founders(0, p, 0, 2 * n, 52 + p)
    sim = Simulation(ctx, 4242, 1, True, device_pedigree=True)
    sim.ras_initial_human_gen0(0, n)
    base = [(0.5, 0.1, 0.1, 0.2, 0.1), (0.4, 0.0, 0.2, 0.3, 0.1)]
    beta = [1.0, 1.0]
    sim.generation_phenotypes(0, 0, [b + (1.0,) for b in base])
    r = sim.phenotypes_result(0)
    beta = [adjusted_beta(r["var"][p], base[p][4], 1) for p in range(2)]
    ctx.compute_selection(0, 0, "none", 0, 0, [1.0, 0.5], [1.0, 1.0], want=())
    sim.save_prev_gen(0)
    for g in (1, 2):
        if g == 1:
            sim.next_generation_am_selected(0, n, 0.3, 0.1, True, "p")
        else:
            sim.next_generation_rm_selected(0, n)
        sim.generation_phenotypes(0, g, [b + (beta[p],) for p, b in enumerate(base)])
        ctx.compute_selection(0, g, "logit", 0.2, 0.8, [1.0, 0.5], [1.0, 1.0], want=())
        sim.phenotypes_result(0)
        txt = check_text(ctx, 0, sim.sex[0], 2, f"generation {g}", slices=(g == 2))
        assert txt.count(b"\n") == ctx.pop_size(0) + 1
        sim.save_prev_gen(0)
    ctx.close()


def test_text_behind_a_migration(gpu_lib):
    """two populations, one gev_migrate with unequal moves: the rows arrive with the migrants, who keep the ids of their origin"""
    n, k01, k10 = 500, 23, 9
    cfg = SyntheticConfig(n, 1024, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=60, seed=8)
    ctx = gpu_lib.create(2, 1, 1)
    for ip in range(2):
        cfg.apply_static(ctx, ip)
        ctx.synth_founders(ip, 0, 2 * n, 61 + ip)
        ctx.synth_cv_founders(ip, 0, 0, 2 * n, 71 + ip)
    sim = Simulation(ctx, 31337, 1, True, device_pedigree=True)
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
    before = []
    for ip in range(2):
        sim.next_generation_rm_selected(ip, n)
        sim.generation_phenotypes(ip, 1, [base + (beta[ip],)])
        sim.phenotypes_result(ip)
        ctx.compute_selection(ip, 1, "logit", 0.0, 1.0, [1.0], [1.0], want=())
        before.append(check_text(ctx, ip, sim.sex[ip], 1, f"population {ip} before the migration", slices=False).split(b"\n")[1:-1])
    rs = np.random.default_rng(12)
    moves = [(0, int(p), 1) for p in sorted(rs.choice(n, k01, replace=False), reverse=True)] + [(1, int(p), 0) for p in sorted(rs.choice(n, k10, replace=False), reverse=True)]
    old_sex = [sim.sex[0].copy(), sim.sex[1].copy()]
    sim.ras_do_migration(moves)
    for ip in range(2):
        gone = np.zeros(n, dtype=bool)
        gone[[pos for sp, pos, dp in moves if sp == ip]] = True
        keep = np.flatnonzero(~gone)
        came = np.array([pos for sp, pos, dp in moves if dp == ip])
        sex = np.concatenate([old_sex[ip][keep], old_sex[1 - ip][came]])
        assert ctx.pop_size(ip) == len(sex) != n
        got = check_text(ctx, ip, sex, 1, f"population {ip} behind the migration").split(b"\n")[1:-1]
        assert got == [before[ip][i] for i in keep] + [before[1 - ip][i] for i in came], "the migrants' rows, origin ids included, arrive unchanged"
    ctx.close()


def test_info_text_refusals(gpu_lib):
    n = 300
    cfg = SyntheticConfig(n, 1024, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=50, seed=2)

    def population(track, gen0=True):
        ctx = gpu_lib.create(1, 1, 1)
        cfg.apply_static(ctx)
        ctx.synth_founders(0, 0, 2 * n, 3); ctx.synth_cv_founders(0, 0, 0, 2 * n, 4)
        sim = Simulation(ctx, 11, 1, True, device_pedigree=track)
        if gen0:
            sim.ras_initial_human_gen0(0, n)
        return ctx, sim

    def refused(call, word):
        with pytest.raises(capi.GevError) as e:
            call()
        assert word in str(e.value), str(e.value)
        return e.value.code

    scheme = [(0.5, 0.0, 0.1, 0.3, 0.0, 1.0)]
    off, _ = population(False)
    assert refused(lambda: off.format_info_text(0), "track pedigree") == -2
    off.close()
    empty, _ = population(True, gen0=False)
    assert refused(lambda: empty.format_info_text(0, 0, 0), "no current generation") == -2
    empty.close()
    ctx, sim = population(True)
    assert refused(lambda: ctx.format_info_text(0), "no phenotype components") == -2
    sim.generation_phenotypes(0, 0, scheme)
    assert refused(lambda: ctx.format_info_text(0), "outstanding") == -2
    sim.phenotypes_result(0)
    assert refused(lambda: ctx.format_info_text(0), "no selection values") == -2
    ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0], want=())
    assert len(ctx.format_info_text(0)) > n * 30
    assert refused(lambda: ctx.format_info_text(0, n - 1, 2), "beyond") == -1
    assert refused(lambda: ctx.format_info_text(0, n + 1, 0), "beyond") == -1
    rc = ctx.L._f("format_info_text")(ctx.h, 0, 0, n, 1, None, 0, None)
    assert rc == -1 and "bytes_written" in ctx.L.last_error()
    ctx.remove_rows(0, np.array([1, 2], dtype=np.uint64))
    assert refused(lambda: ctx.format_info_text(0), "ids were dropped") == -2
    ctx.close()
    many = gpu_lib.create(1, 1, 9)                                        # 64 rows of 9 phenotypes do not fit the staging area
    assert refused(lambda: many.format_info_text(0, 0, 0), "at most 8") == -5
    many.close()
