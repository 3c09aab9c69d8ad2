"""The lane layout of the batched sampling kernel's map scan (k_sample_batched, csrc/gev_sample8.h: lane (g, j) owns draws
j, j + 8, .. of task g; one exact engine state per lane and block of 2048 draws; steps of four multipliers, i.e. 32 draws per
task) at the shapes where it can go wrong: draw counts around the 8-draw lane stride, the 32-draw step and the 2048-draw block,
task counts around a batch of eight, lane groups with different maps in one wave, empty and all-candidate ranges, and hits
placed on chosen draws.  Every case runs the batched kernel, the one-task-per-wave kernels (GEV_SAMPLE_BATCHED=0) and the CPU
oracle side by side and compares sexes, A/D bits, interval and mutation lists and genotypes.  Nothing has a tolerance.

gev_set_rmap refuses a recombination map of one row, so the scan of ONE draw is the mutation scan (two map rows) beside the
smallest recombination map (two rows, two draws)."""
import numpy as np
import pytest

from tests import helpers
from tests import placed_hits as ph
from tests.synth import synth_packed

pytestmark = pytest.mark.gpu

BATCHED, PER_TASK = 1, 2                    # gev_dbg_sampling_path
STEP = ph.STEP


class Chrom:
    """one chromosome whose mutation scan has n draws (n + 1 map rows) and whose crossover scans have max(n, 2) (as many rows);
    every row has the probability `rec` / `mut` (default about 1 / n, capped at 0.3: most gametes have a hit)"""

    def __init__(self, n, rec=None, mut=None, seed=0):
        p = min(0.3, 1.0 / n)
        self.rbp, self.rprob, self.dist = ph.rmap_rows(max(n, 2), p if rec is None else rec)
        self.mbp, self.mrate = ph.mmap_rows(n + 1, int(self.rbp[-1]), p if mut is None else mut)
        bp0, bp_end = int(self.rbp[0]), int(self.rbp[-1])
        self.snps = np.unique(np.linspace(bp0, bp_end - 1, 200).astype(np.int64)).astype(np.uint64)
        rs = np.random.RandomState(100 + seed)
        self.cv_bp = self.snps[::10][:20].copy()
        self.cv_a, self.cv_d = rs.randn(len(self.cv_bp)), 0.3 * rs.randn(len(self.cv_bp))


def _contexts(gpu_lib, oracle_lib, monkeypatch, nchr, setup):
    """(batched, one task per wave, oracle) contexts, each prepared by setup(ctx, is_oracle)"""
    out = []
    for kind in ("batched", "per_task", "oracle"):
        if kind == "per_task":
            monkeypatch.setenv("GEV_SAMPLE_BATCHED", "0")
        else:
            monkeypatch.delenv("GEV_SAMPLE_BATCHED", raising=False)
        ctx = (oracle_lib if kind == "oracle" else gpu_lib).create(1, nchr, 1)
        setup(ctx, kind == "oracle")
        out.append(ctx)
    return out


def _same_state(a, b, chrs, label):
    for x, y in zip(a.compute_ad(0), b.compute_ad(0)):
        assert helpers.bits_equal(x, y), f"{label}: A/D"
    for c in chrs:
        pa, oa = a.download_intervals(0, c); pb, ob = b.download_intervals(0, c)
        assert np.array_equal(oa, ob) and np.array_equal(pa, pb), f"{label}: intervals chr {c}"
        ma, moa = a.download_mutations(0, c); mb, mob = b.download_mutations(0, c)
        assert np.array_equal(moa, mob) and np.array_equal(ma, mb), f"{label}: mutations chr {c}"
        assert np.array_equal(a.download_haps(0, c), b.download_haps(0, c)), f"{label}: genotypes chr {c}"


def _generations(gpu_lib, oracle_lib, monkeypatch, chroms, n_parents, n_off, n_gen, seed, inactive=()):
    """n_gen generations of n_off offspring (generation 0 has n_parents people) on the three contexts, compared after each.
    Returns the mean number of crossovers per gamete and of new mutations per haplotype row of the last generation."""
    nchr = len(chroms)
    mine = [c for c in range(nchr) if c not in inactive]

    def setup(ctx, is_oracle):
        have = range(nchr) if is_oracle else mine       # the oracle simulates every chromosome and reports the active ones
        for c, ch in enumerate(chroms):
            ctx.set_rmap(0, c, ch.rbp, ch.rprob, ch.dist)
            ctx.set_mutmap(0, c, ch.mbp, ch.mrate)
        for c in have:
            ctx.set_snps(0, c, chroms[c].snps)
            ctx.set_cvs(0, 0, c, chroms[c].cv_bp, chroms[c].cv_a, chroms[c].cv_d, 0.2)
        if inactive:
            for c in range(nchr):
                ctx.set_chr_active(c, c in mine)
        nh = 2 * n_parents
        for c in have:
            L, ncv = len(chroms[c].snps), len(chroms[c].cv_bp)
            if is_oracle:
                ctx.upload_founders(0, c, synth_packed(50 + c, nh, L), L)
                ctx.upload_cv_founders(0, 0, c, synth_packed(60 + c, nh, ncv), ncv)
            else:
                ctx.synth_founders(0, c, nh, 50 + c); ctx.synth_cv_founders(0, 0, c, nh, 60 + c)

    g1, g0, o = _contexts(gpu_lib, oracle_lib, monkeypatch, nchr, setup)
    sex = g1.init_gen0(0, n_parents, seed)
    assert np.array_equal(sex, g0.init_gen0(0, n_parents, seed)) and np.array_equal(sex, o.init_gen0(0, n_parents, seed))
    rng = np.random.default_rng(seed)
    done = 0
    for gen in range(1, n_gen + 1):
        males, females = np.flatnonzero(sex == 1), np.flatnonzero(sex == 2)
        if not (len(males) and len(females)):
            break                           # (a generation of one or two people may have one sex only)
        couples = np.zeros((n_off, 4), dtype=np.int64)
        couples[:, 0] = males[rng.integers(0, len(males), n_off)]
        couples[:, 1] = females[rng.integers(0, len(females), n_off)]
        couples[:, 3] = 1
        seed_reproduce = int(rng.integers(1, 2 ** 31))
        mut_seeds = rng.integers(1, 2 ** 32, n_off * nchr, dtype=np.uint64).astype(np.uint32)
        sex = g1.reproduce(0, couples, seed_reproduce, mut_seeds)
        assert g1.dbg_sampling_path() == BATCHED
        assert np.array_equal(sex, o.reproduce(0, couples, seed_reproduce, mut_seeds)), f"sexes against the oracle, generation {gen}"
        assert np.array_equal(sex, g0.reproduce(0, couples, seed_reproduce, mut_seeds)), f"sexes against one task per wave, generation {gen}"
        assert g0.dbg_sampling_path() == PER_TASK
        _same_state(g1, o, mine, f"oracle, generation {gen}")
        _same_state(g1, g0, mine, f"one task per wave, generation {gen}")
        done += 1
    assert done >= 1
    parts = sum(len(g1.download_intervals(0, c)[0]) for c in mine)
    muts = sum(len(g1.download_mutations(0, c)[0]) for c in mine)
    rows = 2 * n_off * len(mine)
    for ctx in (g1, g0, o):
        ctx.close()
    return parts / rows, muts / rows


EDGE_DRAWS = [1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 2056, 4097]


@pytest.mark.parametrize("n", EDGE_DRAWS)
def test_draw_counts_at_the_edges_of_lane_stride_step_and_block(gpu_lib, oracle_lib, monkeypatch, n):
    """n draws per scan (n = 1: see the module's note): fewer than one lane group, a stride of eight with and without a rest, one
    step and one draw more, one block of 2048 exactly, one draw into the second block, a second block whose only step is partial
    (2056) and a third block of one draw.  60 people, three generations, about one event per gamete."""
    parts, muts = _generations(gpu_lib, oracle_lib, monkeypatch, [Chrom(n)], 60, 60, 3, 1000 + n)
    assert parts > 1.2 and muts > 0.1, (parts, muts)        # the maps are hot: pieces per row, new mutations per row


@pytest.mark.parametrize("n_off,nchr", [(1, 1), (7, 1), (8, 1), (9, 1), (17, 1), (3, 3)])
def test_task_counts_around_a_batch_of_eight(gpu_lib, oracle_lib, monkeypatch, n_off, nchr):
    """1, 7, 8, 9, 17 and 3 x 3 tasks: batch 0's lone gamete pass for task 0 with nothing else in the wave, a partial only batch, a
    full one whose gamete pass has seven tasks, and partial last batches of one task"""
    chroms = [Chrom(70 + 9 * c, seed=c) for c in range(nchr)]
    _generations(gpu_lib, oracle_lib, monkeypatch, chroms, 12, n_off, 3, 77 + n_off)


def test_lane_groups_with_different_maps_in_one_wave(gpu_lib, oracle_lib, monkeypatch):
    """three chromosomes of 5, 300 and 2049 draws: the lane groups of a wave alternate between them, so trip counts, first rows,
    thresholds and the number of blocks differ inside one scan loop"""
    chroms = [Chrom(n, seed=i) for i, n in enumerate((5, 300, 2049))]
    _generations(gpu_lib, oracle_lib, monkeypatch, chroms, 50, 50, 3, 31)


def test_lane_groups_with_different_maps_and_an_inactive_chromosome(gpu_lib, oracle_lib, monkeypatch):
    """the same with the longest chromosome in the middle and switched off (gev_set_chr_active): its lane groups run the mutation
    scan for the seed chain and have no gamete scan"""
    chroms = [Chrom(n, seed=i) for i, n in enumerate((5, 2049, 300))]
    _generations(gpu_lib, oracle_lib, monkeypatch, chroms, 50, 50, 3, 32, inactive=(1,))


def test_a_recombination_map_of_zeros_beside_a_live_one(gpu_lib, oracle_lib, monkeypatch):
    """r_amax == 0 on chromosome 0 (no gamete scan in its lane groups, its mutation scan runs), a live map on chromosome 1"""
    chroms = [Chrom(300, rec=0.0, seed=0), Chrom(300, seed=1)]
    assert not chroms[0].rprob.any() and chroms[1].rprob.all()
    _generations(gpu_lib, oracle_lib, monkeypatch, chroms, 50, 50, 3, 33)


def test_every_draw_a_candidate_fills_the_list_in_one_step(gpu_lib, oracle_lib, monkeypatch):
    """one mutation row of probability 0.9999995 in an otherwise cold map of 300 draws: the threshold is at the top of the range,
    all 8 x 32 draws of a step are candidates (a flush behind every step, 256 entries on top of what the list held), and every
    task hits that one row.  The recombination map beside it is warm."""
    ch = Chrom(300, mut=0.0)
    ch.mrate[150] = 0.9999995
    parts, muts = _generations(gpu_lib, oracle_lib, monkeypatch, [ch], 40, 40, 2, 34)
    assert muts >= 0.5                      # one new mutation per task, on one of its two haplotype rows


# ---- placed hits ------------------------------------------------------------------------------------
PLACED_N = 2053                             # draws per scan: 2053 % 8 == 5, the second block holds five draws
PLACED_SINGLES = [0, 7, 8, 2047, 2048, PLACED_N - 1]     # lanes 0 and 7 of the first step, lane 0 of the second multiplier, the last lane
                                                         # of block 0, the first of block 1, the last draw of the map
PLACED_PAIRS = [(2, 3), (44, 45), (2049, 2050)]          # lanes j and j + 1 of one task under the same multiplier


def _placed_scenario(ol):
    """a crossover on each draw of PLACED_SINGLES in the paternal gamete of tasks 0, 1, .. (the seeds that produce those gametes
    are searched), a new mutation on each in a task of its own and on both draws of each pair in one task (closed form; the
    pair's second draw by a search over the first one's high digit)"""
    n = PLACED_N
    bp, rprob, dist = ph.rmap_rows(n)
    mbp, mrate = ph.mmap_rows(n + 1, int(bp[-1]))
    n_x = len(PLACED_SINGLES)
    n_ind = n_x + len(PLACED_SINGLES) + len(PLACED_PAIRS) + 1
    mut_seeds = np.array([1000 + 17 * t for t in range(n_ind)], dtype=np.int64)
    claims = []
    t = n_x
    for i, d in enumerate(PLACED_SINGLES):
        mut_seeds[t] = ph.solve_seed(d, ph._a_target(i), 2, wrap=bool(i & 1))
        ph._place(ol, mrate, d + 1, int(mut_seeds[t]) + 2, d, True)
        claims.append((t, "mut", d + 1)); t += 1
    for i, (d1, d2) in enumerate(PLACED_PAIRS):
        for a1 in range(ph._a_target(10 + i), ph._a_target(10 + i) + ph.SEARCH_CAP):
            S = ph.solve_seed(d1, a1, 2)
            if ph.digits(S + 2, d2)[0] < ph.SEARCH_BOUND:
                break
        else:
            raise RuntimeError("no seed puts both draws of the pair low")
        mut_seeds[t] = S
        for d in (d1, d2):
            ph._place(ol, mrate, d + 1, S + 2, d, True)
            claims.append((t, "mut", d + 1))
        t += 1
    seed_reproduce = 4242
    for i, d in enumerate(PLACED_SINGLES):
        prod = ph._producer(ol, [(mbp, mrate)], 1, i - 1)
        if i == 0:
            seed_reproduce = S = ph.search_seed(4242, prod, d)
        else:
            mut_seeds[i - 1] = S = ph.search_seed(20_000 * i, prod, d)
        ph._place(ol, rprob, d, prod(S) + 1, d, True)
        claims.append((i, "pat", d))
    sc = ph.Scenario("lanes", n_ind, [(bp, rprob, dist)], [(mbp, mrate)], seed_reproduce, mut_seeds)
    for t, what, row in claims:
        sc.designated.append((t, what, f"row {row}")); sc.claims.append((t, what, "hit", row))
    return sc.predict(ol)


def test_hits_placed_on_chosen_lanes_and_steps(gpu_lib, oracle_lib, monkeypatch):
    """the scenario's own prediction (pure Python on the oracle's kat_* helpers; predict() asserts every placed hit), the
    batched kernel, the one-task-per-wave kernels and the oracle agree on the designated tasks and on everything else"""
    sc = _placed_scenario(oracle_lib)
    g1, g0, o = _contexts(gpu_lib, oracle_lib, monkeypatch, 1, lambda ctx, is_oracle: sc.apply(ctx, synth_packed if is_oracle else None))
    s1, s0, so = sc.reproduce(g1), sc.reproduce(g0), sc.reproduce(o)
    assert g1.dbg_sampling_path() == BATCHED and g0.dbg_sampling_path() == PER_TASK
    assert np.array_equal(s1, sc.sex) and np.array_equal(s1, so) and np.array_equal(s1, s0)
    sc.check_designated(g1, "batched,")
    _same_state(g1, o, [0], "placed hits, oracle")
    _same_state(g1, g0, [0], "placed hits, one task per wave")
    for ctx in (g1, g0, o):
        ctx.close()
