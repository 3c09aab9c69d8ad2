"""A generation's chain from the CV planes to A/D where the wide A/D kernel follows: k_stitch_small counts the columns,
k_cv_newmut_sum applies the new mutations and adds the counts up, k_ad_accumulate_wide computes its terms from them, writes the
frequencies and leaves the counters zero.  Every case runs the library and the CPU oracle side by side (inputs: tests/ad_chain.py;
tests/test_ad_chain_cpu.py shows that the oracle alone satisfies what the cases state about themselves) and compares A/D bit for
bit, the allele frequencies and the resolved CV alleles exactly.  Nothing has a tolerance."""
import numpy as np
import pytest

from geneevolve_amd.host import Simulation
from tests import ad_chain as ac
from tests import helpers

pytestmark = pytest.mark.gpu

CHAIN = ac.WIDE + ac.FROM_COUNTS          # gev_dbg_ad_path: the wide kernel, terms from the column counts


def _pair(gpu_lib, oracle_lib, case):
    g = gpu_lib.create(1, case.nchr, case.nphen); o = oracle_lib.create(1, case.nchr, case.nphen)
    case.apply(g); case.apply(o)
    assert g.dbg_ad_path() == 0
    return g, o


def _same(g, o, case, label):
    for x, y in zip(g.compute_ad(0), o.compute_ad(0)):
        assert helpers.bits_equal(x, y), f"{label}: A/D"
    for p in range(case.nphen):
        for c in range(case.nchr):
            assert np.array_equal(g.get_cv_freq(0, p, c).view(np.uint64), o.get_cv_freq(0, p, c).view(np.uint64)), f"{label}: frequencies, phenotype {p} chr {c}"
            assert np.array_equal(g.download_cv(0, p, c), o.download_cv(0, p, c)), f"{label}: resolved CV alleles, phenotype {p} chr {c}"


def _closed_loop(gpu_lib, oracle_lib, case, gens, label, head_start=True):
    g, o = _pair(gpu_lib, oracle_lib, case)
    sg, so = Simulation(g, 9, case.nchr, case.with_mut), Simulation(o, 9, case.nchr, case.with_mut)
    sg.ras_initial_human_gen0(0, case.n_ind); so.ras_initial_human_gen0(0, case.n_ind)
    if head_start:
        g.set_generation_chain(0)
    for gen in range(1, gens + 1):
        ra = sg.next_generation_rm(0, case.n_ind, want_couples=True); rb = so.next_generation_rm(0, case.n_ind, want_couples=True)
        assert ra["glob_state"] == rb["glob_state"] and np.array_equal(ra["couples"], rb["couples"]) and np.array_equal(ra["sex"], rb["sex"]), f"{label}: generation {gen}"
        assert g.dbg_ad_path() == CHAIN, f"{label}: generation {gen} took A/D path {g.dbg_ad_path()}"
        _same(g, o, case, f"{label}, generation {gen}")
    return g, o, sg, so


# individuals: 130 = one k_stitch_small block, half empty; 300 = three blocks of partial counts (fewer than the eight-wide loop);
# 2100 = 17 blocks (uneven slices of the reduction) and a last A/D block that is partly dead.  CV columns: 1, 128, 512 (one piece
# when only A-terms are needed, two otherwise), 513 (a piece with one CV behind them), 1000.
@pytest.mark.parametrize("vd", [0.0, 0.5])
@pytest.mark.parametrize("ncv", [1, 128, 512, 513, 1000])
@pytest.mark.parametrize("n_ind", [130, 300, 2100])
def test_shapes(gpu_lib, oracle_lib, n_ind, ncv, vd):
    g, o, _, _ = _closed_loop(gpu_lib, oracle_lib, ac.Case(n_ind, ncv, vd=(vd,)), 2, f"{n_ind} x {ncv}, vd {vd}")
    g.close(); o.close()


def test_four_work_entries_and_a_cv_behind_the_chromosome_end(gpu_lib, oracle_lib):
    """two phenotypes (vd = 0 and vd > 0) x two chromosomes, every CV grid of another length, the last CV of each uncovered"""
    case = ac.Case(300, [[128, 513], [97, 1000]], vd=(0.0, 0.5), nchr=2, uncovered=True)
    g, o, _, _ = _closed_loop(gpu_lib, oracle_lib, case, 3, "four work entries")
    g.close(); o.close()


@pytest.mark.parametrize("vd", [0.0, 0.5])
def test_without_a_mutation_map(gpu_lib, oracle_lib, vd):
    """the launch behind the stitch has only its reducing blocks"""
    g, o, _, _ = _closed_loop(gpu_lib, oracle_lib, ac.Case(300, 513, vd=(vd,), with_mut=False), 2, f"no mutation map, vd {vd}")
    g.close(); o.close()


@pytest.mark.parametrize("ncv", [1, 128])
def test_new_mutations_on_cv_positions(gpu_lib, oracle_lib, ncv):
    """gev_reproduce with given mutation seeds: nearly every task hits a CV position, some hit one twice on the same haplotype; the
    hits the scan arithmetic predicts are in the library's lists, and everything equals the oracle for three generations"""
    case = ac.Case(130, ncv)
    g, o = _pair(gpu_lib, oracle_lib, case)
    assert np.array_equal(g.init_gen0(0, case.n_ind, 77), o.init_gen0(0, case.n_ind, 77))
    for gen in (1, 2, 3):
        sg = g.reproduce(0, case.couples(), 500 + gen, case.mut_seeds(gen)); so = o.reproduce(0, case.couples(), 500 + gen, case.mut_seeds(gen))
        assert np.array_equal(sg, so), f"generation {gen}: sexes"
        assert g.dbg_ad_path() == CHAIN, f"generation {gen} took A/D path {g.dbg_ad_path()}"
        hits = case.predicted_hits(oracle_lib, gen)
        assert ac.repeated_hits(hits)
        muts, moff = g.download_mutations(0, 0)
        for t, hs in hits.items():
            for x, side in hs:
                row = 2 * t + side
                assert x in [int(v) for v in muts[int(moff[row]):int(moff[row + 1])]], (gen, t, x, side)
        mo, moo = o.download_mutations(0, 0)
        assert np.array_equal(muts, mo) and np.array_equal(moff, moo)
        _same(g, o, case, f"{ncv} CVs, generation {gen}")
    g.close(); o.close()


@pytest.mark.parametrize("vd", [0.0, 0.5])
def test_counters_are_zero_for_whoever_adds_next(gpu_lib, oracle_lib, monkeypatch, vd):
    """five generations closed loop with record regions and list arenas that are too small on purpose (generations are enqueued
    again), and between two of them a stand-alone gev_compute_ad of the current generation after people have left: it counts the
    planes itself (k_cv_count) into the counters the generation's A/D kernel has left"""
    monkeypatch.setenv("GEV_OVF_CAP", "8"); monkeypatch.setenv("GEV_LIST_HEADROOM", "0")      # read when a context is created
    case = ac.Case(300, 513, vd=(vd,), rec=0.25)
    g, o, sg, so = _closed_loop(gpu_lib, oracle_lib, case, 2, f"vd {vd}")
    gone = [3, 10, 57, 299]
    g.remove_rows(0, gone); o.remove_rows(0, gone)
    sg.sex[0] = np.delete(sg.sex[0], gone); so.sex[0] = np.delete(so.sex[0], gone)
    _same(g, o, case, "stand-alone A/D")
    assert g.dbg_ad_path() == ac.WIDE, f"stand-alone A/D took path {g.dbg_ad_path()}"
    for gen in (3, 4, 5):
        ra = sg.next_generation_rm(0, case.n_ind, want_couples=True); rb = so.next_generation_rm(0, case.n_ind, want_couples=True)
        assert ra["glob_state"] == rb["glob_state"] and np.array_equal(ra["couples"], rb["couples"]) and np.array_equal(ra["sex"], rb["sex"]), gen
        assert g.dbg_ad_path() == CHAIN
        _same(g, o, case, f"vd {vd}, generation {gen}")
    assert g.redo_count() >= 1, "the undersized buffers were meant to force generations to be enqueued again"
    g.close(); o.close()
