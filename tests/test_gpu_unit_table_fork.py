"""The segment unit table (k_pool_inherit, k_pool_fresh, k_pool_publish) is built on the mating stream, beside the CV planes and
A/D, and joined before the dense stitch and the status block: that is a schedule only.  Shapes where it could go wrong: rows that
are no multiple of 256, a dozen 64-byte segments per row with a partial last one, two chromosomes (blockIdx.y > 0), three
crossovers per gamete (most segments are written: the free list turns over within a few generations)."""
import numpy as np
import pytest

from geneevolve_amd.host import Simulation, SyntheticConfig, synthetic_random_mate
from tests import helpers
from tests.synth import synth_packed

pytestmark = pytest.mark.gpu

N, L, NCHR, SEED_F, SIM_SEED = 1500, 6000, 2, 70, 8


def _cfg(seed):
    return SyntheticConfig(N, L, nchr=NCHR, chrom_bp=1_000_000, map_step=5_000, rec_per_row=0.015, mut_per_row=0.01, n_cv=50, seed=seed)


def _gpu(gpu_lib, cfg):
    g = gpu_lib.create(1, NCHR, 1)
    cfg.apply_static(g)
    for c in range(NCHR):
        g.synth_founders(0, c, 2 * N, SEED_F + c); g.synth_cv_founders(0, 0, c, 2 * N, SEED_F + 10 + c)
    return g


def _oracle(oracle_lib, cfg):
    o = oracle_lib.create(1, NCHR, 1)
    cfg.apply_static(o)
    for c in range(NCHR):
        o.upload_founders(0, c, synth_packed(SEED_F + c, 2 * N, L), L)
        ncv = len(cfg.cv[0][c][0])
        o.upload_cv_founders(0, 0, c, synth_packed(SEED_F + 10 + c, 2 * N, ncv), ncv)
    return o


def _state(ctx):
    """dense rows, interval lists and mutation lists of both chromosomes"""
    out = []
    for c in range(NCHR):
        out.append(ctx.download_haps(0, c)); out.extend(ctx.download_intervals(0, c)); out.extend(ctx.download_mutations(0, c))
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"{what}: state array {i}"


def _planes_ok(g, what):
    for c in range(NCHR):
        assert g.dbg_verify_planes(0, c, SEED_F + c) == (0, 0), f"{what}: dense rows != materialised intervals (chr {c})"


def _bench_loop(ctx, sim, n_gen, checkpoints, at_checkpoint, hand_over_first=True):
    """bench.py's order of calls: generation g + 1 is begun before generation g's A/D is read (except where the state is read).
    The oracle computes a generation inside generation_begin: it reads A/D first (hand_over_first=False), the values are the same."""
    rec = []
    begun = False
    for gen in range(1, n_gen + 1):
        if not begun:
            ctx.generation_begin(0, sim.glob.x, N)
        r = ctx.generation_end(want_couples=False)
        sim.glob.x = int(r["glob_state"]); sim.sex[0] = r["sex"]
        begun = hand_over_first and gen not in checkpoints
        if begun:
            ctx.generation_begin(0, sim.glob.x, N)
        add, dom, _, _ = ctx.compute_ad(0, per_chr=False)
        rec.append((int(r["glob_state"]), int(r["seed_reproduce"]), int(r["seed_mate"]), r["sex"].copy(), add.copy(), dom.copy()))
        if gen in checkpoints:
            at_checkpoint(gen)
    return rec


N_GEN, CHECKPOINTS = 40, (5, 10, 20, 30, 40)


@pytest.fixture(scope="module")
def oracle_run(oracle_lib):
    """the CPU oracle through the same calls, once: per generation (glob_state, seed_reproduce, seed_mate, sexes, A, D), and the
    whole state at the checkpoints (generation 5 for the five-generation runs of the stitch-mode / unshared-rows test, every
    tenth for the 40-generation test)"""
    cfg = _cfg(41)
    o = _oracle(oracle_lib, cfg)
    so = Simulation(o, SIM_SEED, NCHR, True)
    so.ras_initial_human_gen0(0, N)
    states = {}
    rec = _bench_loop(o, so, N_GEN, CHECKPOINTS, lambda gen: states.__setitem__(gen, _state(o)), hand_over_first=False)
    o.close()
    return rec, states


def _same_generation(a, b, what):
    assert a[:3] == b[:3], f"{what}: glob_state / seed_reproduce / seed_mate {a[:3]} != {b[:3]}"
    assert np.array_equal(a[3], b[3]), f"{what}: sexes"
    assert helpers.bits_equal(a[4], b[4]) and helpers.bits_equal(a[5], b[5]), f"{what}: A/D"


def test_overlapped_equals_serialised_equals_oracle(gpu_lib, oracle_run, monkeypatch):
    """40 generations in bench.py's order of calls with the head start across generations, on a default context (unit table on the
    mating stream) and on a serialised one (everything on one stream): seeds, sexes and A/D of every generation, and at every tenth
    the rows, interval lists, mutation lists and stitch totals are the same and the oracle's; the dense rows equal the
    materialised intervals."""
    monkeypatch.setenv("GEV_SEG_CHUNKS", "4")
    want, want_states = oracle_run
    cfg = _cfg(41)
    runs = []
    for overlap in (True, False):
        g = _gpu(gpu_lib, cfg)
        if not overlap:
            g.set_overlap(False)
        g.set_generation_chain(0)
        sg = Simulation(g, SIM_SEED, NCHR, True)
        sg.ras_initial_human_gen0(0, N)
        states, totals = {}, {}

        def check(gen, g=g, states=states, totals=totals, overlap=overlap):
            if gen % 10:
                return
            states[gen] = _state(g); totals[gen] = g.stitch_totals()
            _planes_ok(g, f"overlap {overlap} gen {gen}")
        rec = _bench_loop(g, sg, N_GEN, CHECKPOINTS, check)
        runs.append((rec, states, totals))
        g.close()
    (ra, sa, ta), (rb, sb, tb) = runs
    for gen in range(N_GEN):
        _same_generation(ra[gen], want[gen], f"overlapped vs oracle, generation {gen + 1}")
        _same_generation(rb[gen], want[gen], f"serialised vs oracle, generation {gen + 1}")
    assert sorted(sa) == sorted(sb) == [10, 20, 30, 40]
    for gen in sa:
        _same(sa[gen], want_states[gen], f"overlapped vs oracle, generation {gen}")
        _same(sb[gen], want_states[gen], f"serialised vs oracle, generation {gen}")
        assert ta[gen] == tb[gen], f"stitch totals at generation {gen}: {ta[gen]} != {tb[gen]}"
    w, t, sw, st = ta[40]
    assert 0 < sw < st and st % (40 * 2 * N * NCHR) == 0 and st // (40 * 2 * N * NCHR) >= 8, "several segments per row, some of them shared with the parents"


def test_unit_table_fork_through_rebuilds_and_redos(gpu_lib, oracle_lib, monkeypatch):
    """gev_generation_begin/_end for 30 generations against the oracle with selection values, a population size alternating between
    1500 and 1900 and buffers that are too small on purpose (tiny overflow regions, no list headroom): generations are enqueued
    again inside _end, and the free list of the unit pool is rebuilt several times, on the stream that then builds the unit table.
    The free list running out in the middle of a generation (FLAG_POOL) needs a generation that takes more units than four times
    the last one's and than a quarter of its own segments, from a list that still held that much.  No parameter choice tried at
    this size reached such a redo within 60 generations (0 of 11-31 rebuilds each): this recipe with and without the small
    buffers; sizes alternating 1900/350 at 3 and at 6 crossovers per gamete; 2400/300/300 at 6 and 2400/300/300/300 at 10
    crossovers; sizes growing 300 -> 3000 at 6 crossovers.  So none is asserted; the count is printed."""
    monkeypatch.setenv("GEV_SEG_CHUNKS", "4"); monkeypatch.setenv("GEV_OVF_CAP", "8"); monkeypatch.setenv("GEV_LIST_HEADROOM", "0")
    cfg = _cfg(37)
    g, o = _gpu(gpu_lib, cfg), _oracle(oracle_lib, cfg)
    sg, so = Simulation(g, SIM_SEED, NCHR, True), Simulation(o, SIM_SEED, NCHR, True)
    sg.ras_initial_human_gen0(0, N); so.ras_initial_human_gen0(0, N)
    rng = np.random.default_rng(12)
    for gen in range(1, 31):
        n = 1500 if gen % 2 else 1900
        svf = None if gen % 3 == 0 else rng.uniform(0.2, 1.4, len(sg.sex[0]))
        ra = sg.next_generation_rm(0, n, svf, want_couples=True); rb = so.next_generation_rm(0, n, svf, want_couples=True)
        for k in ("glob_state", "seed_mate", "seed_reproduce", "num_males_mate", "num_females_mate"):
            assert ra[k] == rb[k], (gen, k, ra[k], rb[k])
        assert np.array_equal(ra["couples"], rb["couples"]), f"couples gen {gen}"
        assert np.array_equal(ra["sex"], rb["sex"]), f"sex gen {gen}"
        for x, y in zip(g.compute_ad(0), o.compute_ad(0)):
            assert helpers.bits_equal(x, y), f"A/D gen {gen}"
        if gen % 10 == 0:
            _same(_state(g), _state(o), f"gen {gen}")
            _planes_ok(g, f"gen {gen}")
    rebuilds, pool_redos = g.dbg_pool_stats(0)
    print(f"redone generations {g.redo_count()}, free-list rebuilds {rebuilds}, redos for an exhausted free list {pool_redos}")
    assert g.redo_count() >= 1, "the undersized buffers were meant to force generations to be enqueued again"
    assert rebuilds >= 2, "the free list was meant to turn over"
    g.close(); o.close()


def test_unit_table_fork_with_host_couples_and_presample(gpu_lib, oracle_lib, monkeypatch):
    """gev_reproduce_begin/_end with couples from the host and gev_presample ahead (the first generation's head start precedes any
    generation; a generation whose head start does not match samples on the main stream and the mating stream waits for it)"""
    monkeypatch.setenv("GEV_SEG_CHUNKS", "4")
    cfg = _cfg(35)
    g, o = _gpu(gpu_lib, cfg), _oracle(oracle_lib, cfg)
    sg, so = Simulation(g, 3, NCHR, True), Simulation(o, 3, NCHR, True)
    sg.ras_initial_human_gen0(0, N); so.ras_initial_human_gen0(0, N)
    rng = np.random.default_rng(6)
    seeds = sg.ras_glob_seed(1 + NCHR * N)
    couples = synthetic_random_mate(sg.sex[0], N, rng)                # generation 1: no head start, the attempt samples itself
    for gen in range(1, 11):
        seeds_next = sg.ras_glob_seed(1 + NCHR * N)
        g.reproduce_begin(0, couples, int(seeds[0]), seeds[1:], n_people=N)
        if gen != 5:                                                   # (generation 6 samples itself again)
            sg.presample(0, seeds_next, N)
        sex = g.reproduce_end()
        so.couples[0] = couples
        assert np.array_equal(so.reproduce(0, gen, seeds=seeds, n_people=N), sex), f"sex gen {gen}"
        for x, y in zip(g.compute_ad(0), o.compute_ad(0)):
            assert helpers.bits_equal(x, y), f"A/D gen {gen}"
        couples, seeds = synthetic_random_mate(sex, N, rng), seeds_next
    g.sync()
    _planes_ok(g, "host couples")
    _same(_state(g), _state(o), "host couples")
    g.close(); o.close()


def test_unit_table_fork_with_assortative_generations(gpu_lib, oracle_lib, monkeypatch):
    """gev_generation_begin_assort/_end (mating correlation 0.4, 15 % of the couples married at random, Poisson offspring numbers):
    the oracle breeds from the couples the device formed, with seeds drawn from its own glob stream in the reference's order"""
    monkeypatch.setenv("GEV_SEG_CHUNKS", "4")
    cfg = _cfg(36)
    g, o = _gpu(gpu_lib, cfg), _oracle(oracle_lib, cfg)
    sg, so = Simulation(g, 5, NCHR, True), Simulation(o, 5, NCHR, True)
    sg.ras_initial_human_gen0(0, N); so.ras_initial_human_gen0(0, N)
    rs = np.random.default_rng(9)
    for gen in range(1, 11):
        mv = rs.standard_normal(len(sg.sex[0]))
        r = sg.next_generation_am(0, N, 0.4, 0.15, False, "p", mating_value=mv, want_couples=True)
        so.ras_glob_seed(4)                                            # assort_mate's draws (three and one for the Poisson numbers)
        so.couples[0] = r["couples"]
        sex = so.reproduce(0, gen)
        assert so.glob.x == int(r["glob_state"]) and so.last_seed_reproduce == int(r["seed_reproduce"]), f"seed stream gen {gen}"
        assert np.array_equal(sex, r["sex"]), f"sex gen {gen}"
        for x, y in zip(g.compute_ad(0), o.compute_ad(0)):
            assert helpers.bits_equal(x, y), f"A/D gen {gen}"
    _planes_ok(g, "assortative")
    g.close(); o.close()


@pytest.mark.parametrize("env", ["GEV_STITCH_MODE=1", "GEV_ALIAS_ROWS=0"])
def test_unit_table_fork_with_row_stitch_and_without_shared_rows(gpu_lib, oracle_run, monkeypatch, env):
    """the gamete-major stitch kernel, and rows that share nothing with the parents (k_pool_inherit returns at once, k_pool_fresh
    names every segment): five generations, the oracle's values and state, dense rows == materialised intervals.  Both variables
    are read when the context is created.  Unshared rows show in the stitch totals; the stitch mode has no observable but the
    kernel's name (it reads the same records and writes the same rows), so it is set through gev_set_stitch_mode as well."""
    monkeypatch.setenv("GEV_SEG_CHUNKS", "4"); monkeypatch.setenv(*env.split("="))
    want, want_states = oracle_run
    g = _gpu(gpu_lib, _cfg(41))
    if env == "GEV_STITCH_MODE=1":
        g.set_stitch_mode(1)
    g.set_generation_chain(0)
    sg = Simulation(g, SIM_SEED, NCHR, True)
    sg.ras_initial_human_gen0(0, N)
    got = {}

    def check(gen):
        if gen == 5:
            _planes_ok(g, env); got[5] = _state(g)
    rec = _bench_loop(g, sg, 5, CHECKPOINTS, check)
    for gen in range(5):
        _same_generation(rec[gen], want[gen], f"{env}, generation {gen + 1}")
    _same(got[5], want_states[5], env)
    if env == "GEV_ALIAS_ROWS=0":
        w, t, sw, st = g.stitch_totals()
        assert sw == st, "every segment was meant to be written"
    g.close()
