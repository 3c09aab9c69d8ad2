"""gev_format_interval_text: Simulation::ras_write_hap_to_interval_format's .int file (reference src/Simulation.cpp:1582-1639) written on
the device, byte for byte -- fixture replays against the reference's recorded files, the device against the same header built for the
host at a size that makes the offset scan loop with rows that straddle block edges, behind a migration, and the refusals.
(The library keeps no counter of its device allocations, so "a context that never calls the feature allocates nothing for it" is not
asserted here; the state it would allocate is created in gev_format_interval_text alone.)"""
import numpy as np
import pytest

from geneevolve_amd import capi
from geneevolve_amd.host import Simulation, SyntheticConfig
from tests import helpers
from tests import int_text_inputs as T

pytestmark = pytest.mark.gpu


def first_difference(got, want):
    la, lb = got.split(b"\n"), want.split(b"\n")
    first = next((i for i, (a, b) in enumerate(zip(la, lb)) if a != b), min(len(la), len(lb)))
    return f"{len(got)} bytes vs {len(want)}; first differing line {first}: {la[first:first + 1]} vs {lb[first:first + 1]}"


# ---- the reference's recorded files ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,plane_less", [("mig2", False), ("mig3c", False), ("ex1mut", False), ("om1", False), ("vcf1", False), ("mig2", True)])
def test_replayed_fixture_gives_the_references_int_files(gpu_lib, oracle_lib, case, plane_less):
    """the fixture's generations replayed through the library (recorded couples, seeds and moves); at every generation the reference
    wrote .int files for, every population x chromosome: the device text with the host's ids and with the ids the library tracks
    against the reference's SHA-256.  plane_less: the same on a context without genotype planes (gev_set_dense_state(0))"""
    fx = helpers.load_fixture(case)
    n_pop, nchr, nphen, ngen = int(fx["n_pop"]), int(fx["nchr"]), int(fx["nphen"]), int(fx["n_gen"])
    files = T.recorded_files(fx)
    ctx = gpu_lib.create(n_pop, nchr, nphen)
    if plane_less:
        ctx.set_dense_state(False)
    helpers.setup_static(ctx, fx, snp_founders=not plane_less)
    ctx.set_track_pedigree(True)
    for ip, names in enumerate(T.founder_names(fx)):
        ctx.set_founder_names(ip, names)
    for ip, seed in enumerate(helpers.find_gen0_seeds(fx, oracle_lib)):
        ctx.init_gen0(ip, len(fx[f"g0_pop{ip}_sex"]), seed)
    compared = 0
    for g in range(1, ngen + 1):
        for ip in range(n_pop):
            pre = f"g{g}_pop{ip}_"
            ms = fx[pre + "mut_seeds"]
            sex = ctx.reproduce(ip, fx[pre + "couples"], int(fx[pre + "seed_reproduce"]), ms if len(ms) else None)
            assert np.array_equal(sex, fx[pre + "sex"])
            ctx.compute_ad(ip)
        if f"g{g}_moves" in fx:
            ctx.migrate(helpers.derive_moves(fx, g))
        for key, _, ip, ic, pre, label in [f for f in files if f[1] == g]:
            ids = fx[pre + "ids"][:, 0]
            assert np.array_equal(ctx.download_pedigree(ip)[:, 0], ids), f"{case}: the library's ID plane, generation {g} population {ip}"
            for arg in (ids, None):
                txt = ctx.format_interval_text(ip, ic, label, ids=arg)
                assert np.array_equal(T.sha256(txt), fx[key]), f"{case}: {key} differs from the reference's file (ids {'from the host' if arg is not None else 'of the library'})"
            compared += 1
    assert compared == len(files) > 0
    ctx.close()


# ---- the device against the host build -------------------------------------------------------------------------------------------------
def synth_names(ip, n):
    """lengths 1 to 64 mixed"""
    return [chr(ord("a") + ip) * (1 + (k * 13 + 5 * ip) % 64) for k in range(n)]


def check_population(gpu_lib, ctx, ip, label, names, what, slices=()):
    """whole text (ids of the library and ids from the host) and slices against gev_dbg_format_interval_text_host on the downloads"""
    parts, off = ctx.download_intervals(ip, 0)
    ids = ctx.download_pedigree(ip)[:, 0]
    n = ctx.pop_size(ip)
    want = gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names)
    assert want.count(b"\n") == len(parts) + 1
    for arg in (None, ids):
        got = ctx.format_interval_text(ip, 0, label, ids=arg)
        assert got == want, f"{what}: {first_difference(got, want)}"
    assert ctx.interval_text_size(ip, 0, label) == len(want), f"{what}: size query"
    for a, b in slices:
        w = gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names, header=False, ind_begin=a, n_ind=b - a)
        got = ctx.format_interval_text(ip, 0, label, a, b - a, header=False, ids=ids[a:b])
        assert got == w, f"{what}: individuals [{a},{b}): {first_difference(got, w)}"
        assert ctx.format_interval_text(ip, 0, label, a, b - a, header=False) == w, f"{what}: individuals [{a},{b}), ids of the library"
    return parts, off, want


def test_device_text_equals_the_host_build_at_scale_and_behind_a_migration(gpu_lib):
    """Population 0 breeds on a hot map (about 20 crossovers per gamete and generation), population 1 (3001 individuals) on a cold one;
    160 individuals of population 0 then move to population 1, which breeds once more: a few hundred haplotypes with several hundred
    parts beside thousands with one or two, more parts than 256 blocks of 256 (the offset scan takes more than one round), rows that
    straddle block edges.  Whole text, slices that begin and end inside a block, the copy-out forced into several runs; then the same
    for both populations behind a gev_migrate with unequal moves."""
    n0, n1, gens = 200, 3001, 12
    hot = SyntheticConfig(n0, 1024, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.2, n_cv=20, seed=3, with_mutation=False)
    cold = SyntheticConfig(n1, 1024, chrom_bp=2_000_000, map_step=20_000, rec_per_row=2e-4, n_cv=20, seed=3, with_mutation=False)
    ctx = gpu_lib.create(2, 1, 1)
    for ip, (cfg, n) in enumerate(((hot, n0), (cold, n1))):
        cfg.apply_static(ctx, ip)
        ctx.synth_founders(ip, 0, 2 * n, 81 + ip)
        ctx.synth_cv_founders(ip, 0, 0, 2 * n, 91 + ip)
    names = [synth_names(0, n0), synth_names(1, n1)]
    for ip in range(2):
        ctx.set_founder_names(ip, names[ip])
    sim = Simulation(ctx, 2718, 1, False, device_pedigree=True)
    sim.ras_initial_human_gen0(0, n0); sim.ras_initial_human_gen0(1, n1)
    for g in range(gens):
        sim.next_generation_rm(0, n0)
    rs = np.random.default_rng(4)
    sim.ras_do_migration([(0, int(p), 1) for p in sorted(rs.choice(n0, 160, replace=False), reverse=True)])
    sim.next_generation_rm(1, n1)
    label = 22
    parts, off, want = check_population(gpu_lib, ctx, 1, label, names, "population 1")
    per_row = np.diff(off.astype(np.int64))
    n_blocks = -(-len(parts) // 256)
    print(f"{len(parts)} parts in {n_blocks} blocks; {int((per_row <= 2).sum())} rows with one or two parts, {int((per_row >= 200).sum())} with 200 or more, longest {int(per_row.max())}")
    assert n_blocks > 256 and (per_row <= 2).sum() > 1000 and (per_row >= 200).sum() >= 10
    # slices whose first and last part lie inside a block (not at a multiple of 256 parts), one of them within a single long row's block
    edges = [int(i) for i in np.flatnonzero(off[0::2] % 256 != 0)]
    long_ind = int(np.argmax(per_row)) // 2
    slices = [(edges[1], edges[len(edges) // 2]), (edges[len(edges) // 2], edges[-1]), (long_ind, long_ind + 1), (n1 - 1, n1), (0, 1)]
    ids = ctx.download_pedigree(1)[:, 0]
    for a, b in slices:
        w = gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names, header=False, ind_begin=a, n_ind=b - a)
        assert ctx.format_interval_text(1, 0, label, a, b - a, header=False) == w, f"individuals [{a},{b})"
        assert ctx.format_interval_text(1, 0, label, a, b - a, header=False, ids=ids[a:b]) == w, f"individuals [{a},{b}), ids from the host"
    ctx.dbg_output_chunk(7)                                   # the text leaves in runs of at most 7 blocks: many runs, the last one ragged
    got = ctx.format_interval_text(1, 0, label)
    ctx.dbg_output_chunk(0)
    assert got == want, f"copy-out in runs of 7 blocks: {first_difference(got, want)}"
    # a migration with unequal moves in both directions
    m0, m1 = ctx.pop_size(0), ctx.pop_size(1)
    moves = [(1, int(p), 0) for p in sorted(rs.choice(m1, 37, replace=False), reverse=True)] + [(0, int(p), 1) for p in sorted(rs.choice(m0, 11, replace=False), reverse=True)]
    before = [ctx.format_interval_text(ip, 0, label).split(b"\n")[1:-1] for ip in range(2)]
    sim.ras_do_migration(moves)
    assert ctx.pop_size(0) == m0 + 26 and ctx.pop_size(1) == m1 - 26
    for ip in range(2):
        n = ctx.pop_size(ip)
        check_population(gpu_lib, ctx, ip, label, names, f"population {ip} behind the migration", slices=((0, n // 3), (n // 3, n - 5), (n - 5, n)))
    after = [ctx.format_interval_text(ip, 0, label).split(b"\n")[1:-1] for ip in range(2)]
    assert sorted(after[0] + after[1]) == sorted(before[0] + before[1]), "every line, origin ids included, arrives unchanged"
    ctx.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_interval_text_refusals(gpu_lib):
    n = 300
    cfg = SyntheticConfig(n, 1024, chrom_bp=2_000_000, map_step=20_000, rec_per_row=1e-3, n_cv=50, seed=2, with_mutation=False)

    def population(track, names=True):
        ctx = gpu_lib.create(1, 1, 1)
        cfg.apply_static(ctx)
        ctx.synth_founders(0, 0, 2 * n, 3); ctx.synth_cv_founders(0, 0, 0, 2 * n, 4)
        sim = Simulation(ctx, 11, 1, False, device_pedigree=track)
        sim.ras_initial_human_gen0(0, n)
        if names:
            ctx.set_founder_names(0, synth_names(0, n))
        return ctx, sim

    def refused(call, word):
        with pytest.raises(capi.GevError) as e:
            call()
        assert word in str(e.value), str(e.value)
        return e.value.code

    ids = np.arange(n, dtype=np.int64)
    ctx, _ = population(True, names=False)
    assert refused(lambda: ctx.format_interval_text(0, 0, 1), "never set") == -2
    assert refused(lambda: ctx.set_founder_names(0, ["a", "b" * 65]), "64") == -5
    assert refused(lambda: ctx.format_interval_text(0, 0, 1), "never set") == -2          # the refused table was not kept
    ctx.set_founder_names(0, synth_names(0, n - 1))                                          # the last founder has no name
    assert refused(lambda: ctx.format_interval_text(0, 0, 1), "beyond the names") == -1
    nb = capi.C.c_size_t(77)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    rc = ctx.L._f("format_interval_text")(ctx.h, 0, 0, 1, 0, n, 1, None, buf, len(buf), capi.C.byref(nb))
    assert rc == -1 and nb.value == 0 and not buf.any(), "no text is returned"
    assert ctx.format_interval_text(0, 0, 1, 0, n - 1).count(b"\n") == 2 * (n - 1) + 1       # the named ones alone are fine
    ctx.set_founder_names(0, synth_names(0, n))
    want = ctx.format_interval_text(0, 0, 1)
    assert want.count(b"\n") == 2 * n + 1 and want == ctx.format_interval_text(0, 0, 1, ids=ids)
    assert ctx.format_interval_text(0, 0, 1, 0, 0) == T.HEADER and ctx.format_interval_text(0, 0, 1, 0, 0, header=False) == b""
    assert ctx.format_interval_text(0, 0, 1, n, 0, header=False) == b""
    assert refused(lambda: ctx.format_interval_text(0, 0, 1, n - 1, 2), "beyond") == -1
    assert refused(lambda: ctx.format_interval_text(0, 0, 1, n + 1, 0), "beyond") == -1
    rc = ctx.L._f("format_interval_text")(ctx.h, 0, 0, 1, 0, n, 1, None, None, 0, None)
    assert rc == -1 and "bytes_written" in ctx.L.last_error()
    buf = np.zeros(len(want), dtype=np.uint8)
    rc = ctx.L._f("format_interval_text")(ctx.h, 0, 0, 1, 0, n, 1, None, buf, len(want) - 1, capi.C.byref(nb))
    assert rc == -1 and nb.value == len(want), "one byte too few"
    rc = ctx.L._f("format_interval_text")(ctx.h, 0, 0, 1, 0, n, 1, None, buf, len(want), capi.C.byref(nb))
    assert rc == 0 and buf.tobytes() == want, "a buffer of exactly the size"
    ctx.remove_rows(0, np.array([1, 2], dtype=np.uint64))
    assert refused(lambda: ctx.format_interval_text(0, 0, 1), "dropped") == -2
    kept = np.delete(ids, [1, 2])
    lines = want.split(b"\n")
    assert ctx.format_interval_text(0, 0, 1, ids=kept) == b"\n".join(lines[:3] + lines[7:])   # with the host's ids it still works
    ctx.set_track_intervals(False)
    assert refused(lambda: ctx.format_interval_text(0, 0, 1, ids=kept), "interval tracking") == -2
    ctx.close()
    off, _ = population(False)
    assert refused(lambda: off.format_interval_text(0, 0, 1), "does not track pedigree") == -2
    assert off.format_interval_text(0, 0, 1, ids=ids) == want
    off.close()
