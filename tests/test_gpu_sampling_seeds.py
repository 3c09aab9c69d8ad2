"""The batched sampling kernel (k_sample_batched, csrc/gev_sample8.h) where its seeding and its candidate prefilter can go wrong:
srand() seeds at the edges of the signed Schrage step in every lane group (srand8 takes that step once per lane, in 32-bit
arithmetic, for its own group's seed), map probabilities at the edges of the prefilter's 16-bit fraction field and on both sides
of its all-candidates switch, and draws whose high digit sits exactly on the map's largest threshold, on the first and the last
lane of a scan step.  Every case runs the batched kernel, the one-task-per-wave kernels (GEV_SAMPLE_BATCHED=0) and the CPU oracle
side by side and compares sexes, A/D bits, interval and mutation lists and genotypes.  Nothing has a tolerance."""
import numpy as np
import pytest

from tests import placed_hits as ph
from tests.synth import synth_packed
from tests.test_gpu_sampling_lanes import BATCHED, PER_TASK, Chrom, _contexts, _same_state

pytestmark = pytest.mark.gpu


def _run(gpu_lib, oracle_lib, monkeypatch, ch, n_parents, n_off, plan, seed):
    """one chromosome `ch`, generation 0 of n_parents people, then one generation of n_off offspring per entry
    (seed_reproduce, mut_seeds) of `plan` on the three contexts, compared after each.
    Returns (crossovers, new mutations) of the first generation, counted on the batched context."""
    def setup(ctx, is_oracle):
        ctx.set_rmap(0, 0, ch.rbp, ch.rprob, ch.dist)
        ctx.set_mutmap(0, 0, ch.mbp, ch.mrate)
        ctx.set_snps(0, 0, ch.snps)
        ctx.set_cvs(0, 0, 0, ch.cv_bp, ch.cv_a, ch.cv_d, 0.2)
        nh, L, ncv = 2 * n_parents, len(ch.snps), len(ch.cv_bp)
        if is_oracle:
            ctx.upload_founders(0, 0, synth_packed(50, nh, L), L)
            ctx.upload_cv_founders(0, 0, 0, synth_packed(60, nh, ncv), ncv)
        else:
            ctx.synth_founders(0, 0, nh, 50); ctx.synth_cv_founders(0, 0, 0, nh, 60)

    g1, g0, o = _contexts(gpu_lib, oracle_lib, monkeypatch, 1, setup)
    sex = g1.init_gen0(0, n_parents, seed)
    assert np.array_equal(sex, g0.init_gen0(0, n_parents, seed)) and np.array_equal(sex, o.init_gen0(0, n_parents, seed))
    rng = np.random.default_rng(seed)
    first = None
    for gen, (seed_reproduce, mut_seeds) in enumerate(plan, 1):
        males, females = np.flatnonzero(sex == 1), np.flatnonzero(sex == 2)
        assert len(males) and len(females), "the generation has one sex only: choose another seed"
        couples = np.zeros((n_off, 4), dtype=np.int64)
        couples[:, 0] = males[rng.integers(0, len(males), n_off)]
        couples[:, 1] = females[rng.integers(0, len(females), n_off)]
        couples[:, 3] = 1
        mut_seeds = np.asarray(mut_seeds, dtype=np.uint32)
        assert len(mut_seeds) == n_off
        sex = g1.reproduce(0, couples, seed_reproduce, mut_seeds)
        assert g1.dbg_sampling_path() == BATCHED
        assert np.array_equal(sex, o.reproduce(0, couples, seed_reproduce, mut_seeds)), f"sexes against the oracle, generation {gen}"
        assert np.array_equal(sex, g0.reproduce(0, couples, seed_reproduce, mut_seeds)), f"sexes against one task per wave, generation {gen}"
        assert g0.dbg_sampling_path() == PER_TASK
        _same_state(g1, o, [0], f"oracle, generation {gen}")
        _same_state(g1, g0, [0], f"one task per wave, generation {gen}")
        if first is None:                   # generation 0 has one piece per row and no new mutation
            first = (len(g1.download_intervals(0, 0)[0]) - 2 * n_off, len(g1.download_mutations(0, 0)[0]))
    for ctx in (g1, g0, o):
        ctx.close()
    return first


# ---- seeds at the edges of the signed Schrage step ----------------------------------------------------
# srand(0) seeds like srand(1); 2^31 - 1 = M gives r_1 = 0; from 2^31 on the seed enters as a negative int32
EDGE_SEEDS = [0, 1, 2, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1]
SEED_TASKS = 17                             # two batches of eight and one task
SEED_SHIFTS = [(0, 1), (2, 3), (4, 5), (6, 7)]      # the shift of the cycle in the two generations of a case


def _cycled(shift):
    return [EDGE_SEEDS[(t + shift) % len(EDGE_SEEDS)] for t in range(SEED_TASKS)]


def test_the_shifted_cycles_put_every_seed_on_every_lane_group():
    """(no GPU work) over the eight shifts every edge seed is the mutation seed of a task in each of the eight positions t mod 8,
    i.e. enters srand8 in every lane group; the gamete seeds behind them are rand() outputs of those streams"""
    seen = {(s, t % 8) for a, b in SEED_SHIFTS for shift in (a, b) for t, s in enumerate(_cycled(shift))}
    assert seen == {(s, g) for s in EDGE_SEEDS for g in range(8)}


@pytest.mark.parametrize("seed_reproduce", [1, 2 ** 31 - 1])
@pytest.mark.parametrize("shifts", SEED_SHIFTS)
def test_seeds_at_the_edges_of_the_signed_schrage_step(gpu_lib, oracle_lib, monkeypatch, shifts, seed_reproduce):
    """17 offspring, one chromosome of 64 draws with hot maps, two generations whose mutation seeds cycle through EDGE_SEEDS"""
    plan = [(seed_reproduce, _cycled(s)) for s in shifts]
    xo, muts = _run(gpu_lib, oracle_lib, monkeypatch, Chrom(64), 12, SEED_TASKS, plan, 500 + shifts[0])
    assert xo > 0 and muts > 0, (xo, muts)  # the maps are hot: the streams behind the seeds are used


# ---- map probabilities at the edges of the 16-bit prefilter field ----------------------------------------
U16 = 1.0 / 65536.0
EDGE_PROBS = ([k * U16 + e for k in (1, 2, 33) for e in (-1e-9, 0.0, 1e-9)]     # floor(amax 2^16 / M) on either side of k
              + [1e-7]                                                          # floor() = 0: only the margin is left
              + [1.0 - m * U16 for m in range(1, 13)])                          # both sides of the all-candidates switch


@pytest.mark.parametrize("which,n,d", [("mut", 65, 40), ("mut", 2049, 2048), ("rec", 65, 40), ("rec", 2049, 2040)])
def test_probabilities_at_the_edges_of_the_prefilter_field(gpu_lib, oracle_lib, monkeypatch, which, n, d):
    """one designated row (under draw d: lane 0 of the second step, the only draw of the second block, lane 0 under the last
    multiplier of the first block; a crossover on a map's last row leaves no piece behind it and could not be counted) in an
    otherwise cold mutation or recombination map of n draws; the other map is warm.  20 offspring, one generation per probability."""
    hits = 0
    for i, p in enumerate(EDGE_PROBS):
        ch = Chrom(n, mut=0.0) if which == "mut" else Chrom(n, rec=0.0)
        if which == "mut":
            ch.mrate[d + 1] = p             # draw d of the mutation scan tests row d + 1
        else:
            ch.rprob[d] = p
        rs = np.random.default_rng(9000 + 100 * n + i)
        mut_seeds = rs.integers(0, 2 ** 32, 20, dtype=np.uint64)
        xo, muts = _run(gpu_lib, oracle_lib, monkeypatch, ch, 12, 20, [(int(rs.integers(1, 2 ** 31)), mut_seeds)], 600 + i)
        got = muts if which == "mut" else xo
        if p > 0.99:
            assert got >= 10, (p, got)      # nearly every task (gamete) hits the designated row
        hits += got
    assert hits > 0


# ---- a draw exactly on the map's largest threshold ----------------------------------------------------
def _threshold_scenario(gl, ol):
    """mutation tasks whose draw d has the high digit a = a_hi - 1 (the last candidate: x2 = amax) and a = a_hi (the first draw that
    is none) of the map's only two warm rows, under draws 32 and 39: lanes 0 and 7 of the second step.  The rows' probability is the
    first of a list at which both draws with a = a_hi - 1 hit (the low digit decides inside the threshold's window), so a
    prefilter that loses its last candidate loses a hit."""
    R, ds = 70, (32, 39)
    bp, rprob, dist = ph.rmap_rows(R, 1e-3)
    for i in range(400):
        p = 2e-3 * (1.0 + 1e-4 * i)
        a_hi = ph.threshold(gl, p)[1]
        seeds = {(d, a): ph.solve_seed(d, a, 2, wrap=bool(d & 1)) for d in ds for a in (a_hi - 1, a_hi)}
        if all(ph.draw_value(ol, seeds[d, a_hi - 1] + 2, d) < p for d in ds):
            break
    else:
        raise RuntimeError("no probability in the list makes both draws with a = a_hi - 1 hit")
    mbp, mrate = ph.mmap_rows(R + 1, int(bp[-1]))
    for d in ds:
        mrate[d + 1] = p
    n_ind = 10
    mut_seeds = np.array([300 + 7 * t for t in range(n_ind)], dtype=np.int64)
    sc = ph.Scenario("largest threshold", n_ind, [(bp, rprob, dist)], [(mbp, mrate)], 35, mut_seeds)
    for t, (d, a) in enumerate(sorted(seeds), 1):
        mut_seeds[t] = seeds[d, a]
        sc.designated.append((t, "mut", f"draw {d} a = a_hi{'' if a == a_hi else ' - 1'}"))
        sc.claims.append((t, "mut", "miss" if a == a_hi else "hit", d + 1))
    sc.mut_seeds = mut_seeds.astype(np.uint32)
    return sc.predict(ol)


def test_draws_on_the_largest_threshold_on_the_first_and_last_lane_of_a_step(gpu_lib, oracle_lib, monkeypatch):
    """the scenario's own prediction (predict() asserts the placed hits and misses), the batched kernel, the one-task-per-wave
    kernels and the oracle agree on the designated tasks and on everything else"""
    sc = _threshold_scenario(gpu_lib, oracle_lib)
    g1, g0, o = _contexts(gpu_lib, oracle_lib, monkeypatch, 1, lambda ctx, is_oracle: sc.apply(ctx, synth_packed if is_oracle else None))
    s1, s0, so = sc.reproduce(g1), sc.reproduce(g0), sc.reproduce(o)
    assert g1.dbg_sampling_path() == BATCHED and g0.dbg_sampling_path() == PER_TASK
    assert np.array_equal(s1, sc.sex) and np.array_equal(s1, so) and np.array_equal(s1, s0)
    sc.check_designated(g1, "batched,")
    _same_state(g1, o, [0], "largest threshold, oracle")
    _same_state(g1, g0, [0], "largest threshold, one task per wave")
    for ctx in (g1, g0, o):
        ctx.close()
