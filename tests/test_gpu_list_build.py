"""The list-piece builder that plans per thread and copies per workgroup (k_lp_build_plan, csrc/gev_lists.h; GEV_LP_LANES=1,
GEV_LP_LITERAL=0) against the CPU oracle: the interval and mutation lists after EVERY generation, the genotype rows at the end.
The cases sit on both sides of the kernel's descriptor budgets (LPP_IV = 3 intervals, LPP_NEW = 4 new positions per item: an
item over either is built by its own thread), on long pieces, on the edges of the persistent grid, on arenas that overflow, on
the equality cases of recombine's comparisons and on one list kind at a time; the last case demands the same lists and the
same arena cursors from all three builders.  The oracle runs once per scenario and is shared between the cases that use it."""
import numpy as np
import pytest

from geneevolve_amd.host import Simulation, SyntheticConfig, synthetic_random_mate
from tests.synth import synth_packed

pytestmark = pytest.mark.gpu

LPP_IV, LPP_NEW = 3, 4           # the budgets of k_lp_build_plan (csrc/gev_lists.h): when they change, the configurations below change
HOT = dict(chrom_bp=2_000_000, map_step=1000, rec_per_row=5e-3)          # 2001 map rows 1 kb apart: ~10 crossovers per gamete

# name -> (SyntheticConfig arguments, generations, seed of the run)
SCENARIOS = {
    "iv_budget": (dict(n_ind=100, n_loci=1000, mut_per_row=5e-4, n_cv=40, seed=81, **HOT), 4, 181),
    "new_budget": (dict(n_ind=100, n_loci=1000, chrom_bp=2_000_000, map_step=1000, rec_per_row=5e-4, mut_per_row=9e-3, n_cv=40, seed=82), 4, 182),
    "long_hot": (dict(n_ind=60, n_loci=600, mut_per_row=5e-3, n_cv=40, seed=83, **HOT), 12, 183),
    "long_planned": (dict(n_ind=60, n_loci=600, chrom_bp=2_000_000, map_step=1000, rec_per_row=5e-4, mut_per_row=3e-3, n_cv=40, seed=84), 24, 184),
    "no_events": (dict(n_ind=100, n_loci=600, chrom_bp=2_000_000, map_step=1000, rec_per_row=0.0, mut_per_row=0.0, n_cv=40, seed=85), 3, 185),
    "few_items": (dict(n_ind=30, n_loci=600, chrom_bp=2_000_000, map_step=1000, rec_per_row=2e-4, mut_per_row=2e-4, n_cv=40, seed=86), 4, 186),
    "many_items": (dict(n_ind=200, n_loci=1000, mut_per_row=5e-3, n_cv=40, seed=87, **HOT), 3, 187),
    "arena": (dict(n_ind=200, n_loci=5000, nchr=2, mut_per_row=8e-3, n_cv=100, seed=61, **HOT), 6, 62),
    "three_bp": (dict(n_ind=60, n_loci=600, chrom_bp=30000, map_step=3, rec_per_row=6e-4, mut_per_row=4e-4, n_cv=40, seed=65), 8, 66),
    "no_mutmap": (dict(n_ind=100, n_loci=1000, n_cv=40, seed=88, with_mutation=False, **HOT), 4, 188),
    "cold": (dict(n_ind=200, n_loci=5000, chrom_bp=2_000_000, map_step=1000, rec_per_row=2e-4, mut_per_row=2e-3, n_cv=100, seed=63), 8, 64),
}
_reference = {}


def founders(ctx, cfg, device):
    cfg.apply_static(ctx)
    nh = 2 * cfg.n_ind
    for c in range(cfg.nchr):
        if device:
            ctx.synth_founders(0, c, nh, cfg.seed + c)
        else:
            ctx.upload_founders(0, c, synth_packed(cfg.seed + c, nh, cfg.n_loci), cfg.n_loci)
        for p in range(cfg.nphen):
            ncv = len(cfg.cv[p][c][0])
            if device:
                ctx.synth_cv_founders(0, p, c, nh, cfg.seed + 100 + 7 * p + c)
            else:
                ctx.upload_cv_founders(0, p, c, synth_packed(cfg.seed + 100 + 7 * p + c, nh, ncv), ncv)


def reference(oracle_lib, name):
    """the oracle's run of a scenario, once: per generation the couples, the sexes and the lists of every chromosome; the rows at the end"""
    if name not in _reference:
        kw, n_gen, seed = SCENARIOS[name]
        cfg = SyntheticConfig(**kw)
        o = oracle_lib.create(1, cfg.nchr, cfg.nphen)
        founders(o, cfg, device=False)
        so = Simulation(o, seed, cfg.nchr, cfg.with_mutation)
        so.ras_initial_human_gen0(0, cfg.n_ind)
        rng = np.random.default_rng(seed)
        gens = []
        for gen in range(1, n_gen + 1):
            couples = synthetic_random_mate(so.sex[0], cfg.n_ind, rng)
            so.couples[0] = couples
            sex = np.array(so.reproduce(0, gen))
            gens.append(dict(couples=couples, sex=sex, intervals=[o.download_intervals(0, c) for c in range(cfg.nchr)],
                             mutations=[o.download_mutations(0, c) for c in range(cfg.nchr)]))
        haps = [o.download_haps(0, c) for c in range(cfg.nchr)]
        o.close()
        _reference[name] = (cfg, seed, gens, haps)
    return _reference[name]


def drive(gpu_lib, oracle_lib, name, track=True, compare=True):
    """the scenario on the device next to the oracle's record -> per generation (list_stats of chromosome 0, the downloaded lists)"""
    cfg, seed, gens, haps = reference(oracle_lib, name)
    g = gpu_lib.create(1, cfg.nchr, cfg.nphen)
    if not track:
        g.set_track_intervals(False)
    founders(g, cfg, device=True)
    sg = Simulation(g, seed, cfg.nchr, cfg.with_mutation)
    sg.ras_initial_human_gen0(0, cfg.n_ind)
    out = []
    for gen, want in enumerate(gens, 1):
        sg.couples[0] = want["couples"]
        assert np.array_equal(sg.reproduce(0, gen), want["sex"]), f"{name}: sex differs at generation {gen}"
        lists = []
        for c in range(cfg.nchr):
            if track:
                pg, og = g.download_intervals(0, c); po, oo = want["intervals"][c]
                if compare:
                    assert np.array_equal(og, oo) and np.array_equal(pg, po), f"{name}: interval lists differ (gen {gen} chr {c})"
                lists.append((pg, og))
            mg, mog = g.download_mutations(0, c); mo, moo = want["mutations"][c]
            if compare:
                assert np.array_equal(mog, moo) and np.array_equal(mg, mo), f"{name}: mutation lists differ (gen {gen} chr {c})"
            lists.append((mg, mog))
        out.append((g.list_stats(0, 0), lists))
    for c in range(cfg.nchr):
        assert np.array_equal(g.download_haps(0, c), haps[c]), f"{name}: genotype rows differ (chr {c})"
    g.close()
    return out


def knobs(monkeypatch, segs=32, lanes=1, literal=0, arena=0):
    monkeypatch.setenv("GEV_LIST_SEGS", str(segs))
    monkeypatch.setenv("GEV_LP_LANES", str(lanes))
    monkeypatch.setenv("GEV_LP_LITERAL", str(literal))
    if arena:
        monkeypatch.setenv("GEV_LIST_ARENA", str(arena))
    else:
        monkeypatch.delenv("GEV_LIST_ARENA", raising=False)


def range_of(x, bp0, lgw, nseg):
    """lp_seg"""
    x = np.asarray(x, dtype=np.int64)
    return np.where(x <= bp0, 0, np.minimum((x - bp0) >> lgw, nseg - 1))


def geometry(cfg, max_seg):
    """lp_geometry -> (nseg, lgw)"""
    span = int(cfg.rmap_bp[-1]) - int(cfg.rmap_bp[0])
    lgw = 0
    while (span >> lgw) + 1 > max_seg:
        lgw += 1
    return (span >> lgw) + 1, lgw


def first_generation_events(oracle_lib, name, max_seg):
    """Generation 1 of the oracle's run: the founders' lists are one part and no mutation per row, so the parts of an offspring
    row behind its first one start at the gamete's crossover boundaries and its mutations are the new ones.
    -> (boundaries, new mutations) per (row, range), two int arrays [rows][nseg]"""
    cfg, _, gens, _ = reference(oracle_lib, name)
    nseg, lgw = geometry(cfg, max_seg)
    bp0 = int(cfg.rmap_bp[0])
    parts, off = gens[0]["intervals"][0]
    muts, moff = gens[0]["mutations"][0]
    rows = len(off) - 1
    nb = np.zeros((rows, nseg), dtype=np.int64); nn = np.zeros((rows, nseg), dtype=np.int64)
    for r in range(rows):
        st = parts["st"][int(off[r]) + 1:int(off[r + 1])]
        np.add.at(nb[r], range_of(st, bp0, lgw, nseg), 1)
        np.add.at(nn[r], range_of(muts[int(moff[r]):int(moff[r + 1])], bp0, lgw, nseg), 1)
    return nb, nn


@pytest.mark.parametrize("segs", [4, 32, 1])
def test_items_on_both_sides_of_the_interval_budget(gpu_lib, oracle_lib, monkeypatch, segs):
    """Hot map, ~10 crossovers per gamete.  An item (row, range with an event) is planned when its range holds at most
    LPP_IV - 1 = 2 of the gamete's boundaries.  GEV_LIST_SEGS=4 (four ranges of 2^19 bp, ~2.6 boundaries each): of the 737
    items of the oracle's first generation 369 = 50 % are over the budget (counted from the oracle's boundaries, asserted below
    to lie in 30 .. 70 %); 32 (31 ranges, ~0.3 boundaries each): well below it, 36 of 1793 = 2 % over; 1: every item far over
    it (198 of 200)."""
    nb, nn = first_generation_events(oracle_lib, "iv_budget", segs)
    items = (nb > 0) | (nn > 0)
    share = ((nb >= LPP_IV) & items).sum() / items.sum()
    print(f"GEV_LIST_SEGS={segs}: {int(((nb >= LPP_IV) & items).sum())} of {int(items.sum())} items over the interval budget = {share:.3f}")
    assert {4: 0.30 <= share <= 0.70, 32: share < 0.05, 1: share > 0.95}[segs], share
    knobs(monkeypatch, segs=segs)
    drive(gpu_lib, oracle_lib, "iv_budget")


def test_items_on_both_sides_of_the_new_mutation_budget(gpu_lib, oracle_lib, monkeypatch):
    """~18 new mutations per individual on TWO ranges: a (row side, range) pair gets ~4.5 new positions, the budget is LPP_NEW = 4.
    Of the 393 pairs of the oracle's first generation that have any, 184 = 47 % have more than four (asserted below: 30 .. 70 %)."""
    nb, nn = first_generation_events(oracle_lib, "new_budget", 2)
    share = (nn > LPP_NEW).sum() / (nn > 0).sum()
    print(f"{int((nn > LPP_NEW).sum())} of {int((nn > 0).sum())} pairs over the new-mutation budget = {share:.3f}")
    assert 0.30 <= share <= 0.70, share
    knobs(monkeypatch, segs=2)
    drive(gpu_lib, oracle_lib, "new_budget")


@pytest.mark.parametrize("name", ["long_hot", "long_planned"])
def test_long_pieces(gpu_lib, oracle_lib, monkeypatch, name):
    """GEV_LIST_SEGS=1: a piece is a whole list.  long_hot: hot map, 60 individuals, 12 generations -- the pieces pass 100 entries
    (every item is over the interval budget: the per-thread path at length).  long_planned: ~1 crossover and ~3 new mutations per
    gamete for 24 generations, so that most items are planned and the 120 pieces of the one workgroup, ~70 mutation entries
    each at the end, take dozens of copy rounds; a run spans many of them."""
    knobs(monkeypatch, segs=1)
    out = drive(gpu_lib, oracle_lib, name)
    st = out[-1][0]
    if name == "long_hot":
        assert st["interval_entries_last_generation"] > 100 * 120, st
    else:
        assert st["mutation_entries_last_generation"] > 256 * 16, st


def test_no_item_at_all(gpu_lib, oracle_lib, monkeypatch):
    """no recombination, no mutation: the work list is empty, the launch does nothing, every table entry names the parent's piece"""
    knobs(monkeypatch)
    out = drive(gpu_lib, oracle_lib, "no_events")
    for st, _ in out:
        assert st["interval_entries_last_generation"] == 0 and st["mutation_entries_last_generation"] == 0, st


def test_fewer_items_than_one_workgroup(gpu_lib, oracle_lib, monkeypatch):
    """60 rows, ~0.4 crossovers and ~0.2 new mutations per row: a few dozen items, most threads of the one workgroup idle"""
    knobs(monkeypatch)
    out = drive(gpu_lib, oracle_lib, "few_items")
    nb, nn = first_generation_events(oracle_lib, "few_items", 32)
    assert 0 < ((nb > 0) | (nn > 0)).sum() < 256
    assert all(0 < st["interval_entries_last_generation"] for st, _ in out)


def test_more_items_than_one_grid_round_and_rows_no_multiple_of_256(gpu_lib, oracle_lib, monkeypatch):
    """400 rows on 31 ranges of the hot map with ~10 new mutations per individual: the grid has ceil(400 * 4 / 256) = 7 workgroups
    = 1792 items per round, the work list is several times as long -- the persistent loop runs, the last round is ragged"""
    knobs(monkeypatch)
    nb, nn = first_generation_events(oracle_lib, "many_items", 32)
    assert ((nb > 0) | (nn > 0)).sum() > 2 * 1792
    drive(gpu_lib, oracle_lib, "many_items")


@pytest.mark.parametrize("segs,arena", [(32, 6), (7, 3)])
def test_arenas_that_overflow(gpu_lib, oracle_lib, monkeypatch, segs, arena):
    """arenas of 6 / 3 entries per row fill up every few generations: the items that do not fit raise the flag and are not copied,
    the arena is compacted and the generation enqueued again -- the lists equal the oracle's after every generation"""
    knobs(monkeypatch, segs=segs, arena=arena)
    out = drive(gpu_lib, oracle_lib, "arena")
    assert out[-1][0]["compactions"] >= 2, out[-1][0]


@pytest.mark.parametrize("segs", [5, 7, 32])
def test_equality_cases_on_a_three_bp_map(gpu_lib, oracle_lib, monkeypatch, segs):
    """map rows 3 bp apart: breakpoints of different generations coincide all the time (zero-length parts, parts that start exactly
    at a boundary, boundaries and mutations on range edges)"""
    knobs(monkeypatch, segs=segs)
    drive(gpu_lib, oracle_lib, "three_bp")


def test_mutation_pieces_only(gpu_lib, oracle_lib, monkeypatch):
    """interval tracking off: no interval piece is planned, allocated or copied"""
    knobs(monkeypatch)
    drive(gpu_lib, oracle_lib, "iv_budget", track=False)
    knobs(monkeypatch, segs=4)
    drive(gpu_lib, oracle_lib, "iv_budget", track=False)


def test_interval_pieces_only(gpu_lib, oracle_lib, monkeypatch):
    """no mutation map: no mutation is drawn (the mutation pieces of the items are empty runs)"""
    knobs(monkeypatch)
    drive(gpu_lib, oracle_lib, "no_mutmap")
    knobs(monkeypatch, segs=4)
    drive(gpu_lib, oracle_lib, "no_mutmap")


@pytest.mark.parametrize("name", ["many_items", "cold"])
def test_every_builder_gives_the_same_lists_and_cursors(gpu_lib, oracle_lib, monkeypatch, name):
    """the planning kernel, the eight-lane kernel and the literal one-lane kernel on a hot and a cold scenario: the placement of a
    piece inside the arena may differ, the lists and the arenas' cursors and entry counts after every generation may not"""
    runs = []
    for lanes, literal in ((1, 0), (8, 0), (1, 1)):
        knobs(monkeypatch, lanes=lanes, literal=literal)
        runs.append(drive(gpu_lib, oracle_lib, name))
    fields = ("rebuilds", "interval_entries_used", "mutation_entries_used", "interval_entries_last_generation", "mutation_entries_last_generation", "compactions")
    for other in runs[1:]:
        for gen, ((st_a, lists_a), (st_b, lists_b)) in enumerate(zip(runs[0], other), 1):
            assert [st_a[f] for f in fields] == [st_b[f] for f in fields], (gen, st_a, st_b)
            for (xa, oa), (xb, ob) in zip(lists_a, lists_b):
                assert np.array_equal(oa, ob) and np.array_equal(xa, xb), f"{name}: lists differ between builders at generation {gen}"
