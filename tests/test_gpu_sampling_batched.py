"""The batched sampling kernel (k_sample_batched, csrc/gev_sample8.h: a generation's mutations and gametes, eight tasks per
wave, slow tasks finished in place) against the one-task-per-wave kernels (GEV_SAMPLE_BATCHED=0) and against the oracle."""
import numpy as np
import pytest

from geneevolve_amd.host import GlobSeedStream, SyntheticConfig, synthetic_random_mate
from tests import helpers
from tests.synth import synth_packed

pytestmark = pytest.mark.gpu


def _lists_equal(a, b, chrs, what):
    for c in chrs:
        pa, oa = a.download_intervals(0, c); pb, ob = b.download_intervals(0, c)
        assert np.array_equal(oa, ob) and np.array_equal(pa, pb), f"intervals {what} chr {c}"
        ma, moa = a.download_mutations(0, c); mb, mob = b.download_mutations(0, c)
        assert np.array_equal(moa, mob) and np.array_equal(ma, mb), f"mutations {what} chr {c}"


def test_batched_sampling_equals_one_task_per_wave_at_config2_size(gpu_lib, monkeypatch):
    """BASELINE config 2 (100k individuals x 1M SNPs, 1000 CVs): three generations through gev_generation_begin / _end with the
    head start across generations, once with the batched kernel and once with GEV_SAMPLE_BATCHED=0.  Seed state, sexes, A/D, the
    interval and mutation lists and every genotype plane word must be the same."""
    n, L, gens = 100_000, 1_000_000, 3
    cfg = SyntheticConfig(n, L, n_cv=1000, seed=12345)
    runs = []
    for batched in ("1", "0"):
        monkeypatch.setenv("GEV_SAMPLE_BATCHED", batched)
        g = gpu_lib.create(1, 1, 1)
        cfg.apply_static(g)
        g.synth_founders(0, 0, 2 * n, 1000)
        g.synth_cv_founders(0, 0, 0, 2 * n, 2000)
        g.init_gen0(0, n, 4242)
        g.set_generation_chain(0)
        state = 987654321
        g.generation_begin(0, state, n)
        out = []
        for gen in range(1, gens + 1):
            r = g.generation_end(want_couples=False, want_sex=True)
            state = int(r["glob_state"])
            if gen < gens:
                g.generation_begin(0, state, n)
            ad = g.compute_ad(0, per_chr=False)
            out.append((r["glob_state"], r["seed_reproduce"], r["seed_mate"], np.array(r["sex"]), ad[0].copy(), ad[1].copy()))
        runs.append((g, out))
    (ga, oa), (gb, ob) = runs
    for gen, (x, y) in enumerate(zip(oa, ob), 1):
        assert x[:3] == y[:3], f"seed state differs at generation {gen}"
        assert np.array_equal(x[3], y[3]), f"sexes differ at generation {gen}"
        assert helpers.bits_equal(x[4], y[4]) and helpers.bits_equal(x[5], y[5]), f"A/D differs at generation {gen}"
    assert np.var(oa[-1][4]) > 0
    _lists_equal(ga, gb, [0], "config 2")
    assert ga.dbg_verify_planes(0, 0, 1000) == (0, 0)
    assert gb.dbg_verify_planes(0, 0, 1000) == (0, 0)
    ga.close(); gb.close()


def test_batched_sampling_equals_one_task_per_wave_with_an_inactive_chromosome(gpu_lib, monkeypatch):
    """three chromosomes of which the middle one is held by another context (gev_set_chr_active): the seed chain runs through
    it, its gametes get empty records.  3001 individuals (9003 tasks: the last wave batch is partial), hot enough maps that
    some tasks take the slow path; sexes, per-chromosome A/D and the lists of the active chromosomes must be the same."""
    cfg = SyntheticConfig(3001, 4000, nchr=3, chrom_bp=2_000_000, map_step=1000, rec_per_row=1.5e-3, mut_per_row=1.5e-3, n_cv=50, seed=21, vd=0.2)
    mine = [0, 2]
    res = []
    for batched in ("1", "0"):
        monkeypatch.setenv("GEV_SAMPLE_BATCHED", batched)
        g = gpu_lib.create(1, 3, 1)
        for c in range(3):
            g.set_rmap(0, c, cfg.rmap_bp, cfg.rmap_prob, cfg.bp_dist)
            g.set_mutmap(0, c, cfg.mut_bp, cfg.mut_rate)
        for c in mine:
            g.set_snps(0, c, cfg.snp_pos)
            bp, a, d = cfg.cv[0][c]
            g.set_cvs(0, 0, c, bp, a, d, cfg.vd)
        for c in range(3):
            g.set_chr_active(c, c in mine)
        for c in mine:
            g.synth_founders(0, c, 2 * cfg.n_ind, 50 + c)
            g.synth_cv_founders(0, 0, c, 2 * cfg.n_ind, 60 + c)
        sex = g.init_gen0(0, cfg.n_ind, 77)
        rng = np.random.default_rng(5)
        seeds = GlobSeedStream(9)
        out = []
        for gen in range(4):
            couples = synthetic_random_mate(sex, cfg.n_ind, rng)
            gs = seeds.draw(1 + 3 * cfg.n_ind)
            sex = g.reproduce(0, couples, int(gs[0]), gs[1:])
            out.append((sex.copy(), [x.copy() for x in g.compute_ad(0)]))
        res.append((g, out))
    (ga, oa), (gb, ob) = res
    for gen, (x, y) in enumerate(zip(oa, ob)):
        assert np.array_equal(x[0], y[0]), f"sexes differ at generation {gen}"
        for u, v in zip(x[1], y[1]):
            assert helpers.bits_equal(u, v), f"A/D differs at generation {gen}"
    _lists_equal(ga, gb, mine, "inactive chromosome")
    ga.close(); gb.close()


def _run_against_oracle(gpu_lib, oracle_lib, cfg, n_gen, seed):
    g = gpu_lib.create(1, cfg.nchr, cfg.nphen); o = oracle_lib.create(1, cfg.nchr, cfg.nphen)
    cfg.apply_static(g); cfg.apply_static(o)
    nh = 2 * cfg.n_ind
    for c in range(cfg.nchr):
        g.synth_founders(0, c, nh, cfg.seed + c); o.upload_founders(0, c, synth_packed(cfg.seed + c, nh, cfg.n_loci), cfg.n_loci)
        ncv = len(cfg.cv[0][c][0])
        g.synth_cv_founders(0, 0, c, nh, cfg.seed + 100 + c); o.upload_cv_founders(0, 0, c, synth_packed(cfg.seed + 100 + c, nh, ncv), ncv)
    sex = g.init_gen0(0, cfg.n_ind, seed)
    assert np.array_equal(sex, o.init_gen0(0, cfg.n_ind, seed))
    rng = np.random.default_rng(seed)
    stream = GlobSeedStream(seed)
    for gen in range(1, n_gen + 1):
        couples = synthetic_random_mate(sex, cfg.n_ind, rng)
        gs = stream.draw(1 + cfg.nchr * cfg.n_ind)
        sex = g.reproduce(0, couples, int(gs[0]), gs[1:])
        assert np.array_equal(sex, o.reproduce(0, couples, int(gs[0]), gs[1:])), f"sex differs at generation {gen}"
        for x, y in zip(g.compute_ad(0), o.compute_ad(0)):
            assert helpers.bits_equal(x, y), f"A/D differs at generation {gen}"
        _lists_equal(g, o, range(cfg.nchr), f"gen {gen}")
        for c in range(cfg.nchr):
            assert np.array_equal(g.download_haps(0, c), o.download_haps(0, c)), f"genotypes gen {gen} chr {c}"
    g.close(); o.close()


@pytest.mark.parametrize("ovf_cap", [None, "8"])
def test_hot_maps_with_many_slow_tasks_match_the_oracle(gpu_lib, oracle_lib, monkeypatch, ovf_cap):
    """about four crossovers per gamete and four new mutations per task (2000 map rows at 2e-3): more than 5 % of the tasks need
    more than the eight precomputed rand() outputs and are finished in place, and about 2 % have more than GEV_BK_CAP / GEV_NM_CAP
    records (overflow regions; with GEV_OVF_CAP=8 the regions run out and the generation is enqueued again)"""
    if ovf_cap:
        monkeypatch.setenv("GEV_OVF_CAP", ovf_cap)
    cfg = SyntheticConfig(500, 3000, nchr=2, chrom_bp=2_000_000, map_step=1000, rec_per_row=2e-3, mut_per_row=2e-3, n_cv=80, seed=17, vd=0.3)
    _run_against_oracle(gpu_lib, oracle_lib, cfg, n_gen=3, seed=4321)


def test_mutation_ranges_that_force_rejections_match_the_oracle(gpu_lib, oracle_lib):
    """a mutation map of two ranges of 1.2e9 bp: uniform_int_distribution<unsigned long> rejects about 44 % of its engine
    outputs there (2147483645 // 1200000001 = 1), so most tasks with a new mutation leave the batched path at the rejection test"""
    cfg = SyntheticConfig(400, 2000, nchr=1, chrom_bp=2_400_000_000, map_step=2_000_000, rec_per_row=1e-3, mut_per_row=0, n_cv=40, seed=23)
    cfg.mut_bp = np.array([1000, 1000 + 1_200_000_000, 1000 + 2_400_000_000], dtype=np.uint64)
    cfg.mut_rate = np.array([0.0, 0.6, 0.6])
    _run_against_oracle(gpu_lib, oracle_lib, cfg, n_gen=3, seed=99)
