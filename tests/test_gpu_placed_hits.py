"""The sampling kernels on placed hits (tests/placed_hits.py): inputs built so that a crossover or a new mutation hangs on the last
bit of one chosen draw -- the first and last draw of a scan, either side of the 64-, 256- and 2048-draw steps, row 0 of a
recombination map, the edge of the candidate prefilter, the counts at which a task leaves the batched fast path, every place in a
wave batch -- through every kernel that can run them.  tests/test_placed_hits_cpu.py shows that the oracle alone satisfies each
stated expectation; here the library must show it on the designated tasks and equal the oracle in everything else.  Nothing has a
tolerance."""
import numpy as np
import pytest

from oracle import oracle_api
from tests import helpers
from tests import placed_hits as ph
from tests.synth import synth_packed

pytestmark = pytest.mark.gpu

BATCHED, PER_TASK, CHAIN_WG, CHAIN_WAVE = 1, 2, 3, 4          # gev_dbg_sampling_path


def _equal_to_oracle(g, o, sc, label):
    for c in range(sc.nchr):
        pg, og = g.download_intervals(0, c); po, oo = o.download_intervals(0, c)
        assert np.array_equal(og, oo) and np.array_equal(pg, po), f"{label}: intervals chr {c}"
        mg, mog = g.download_mutations(0, c); mo, moo = o.download_mutations(0, c)
        assert np.array_equal(mog, moo) and np.array_equal(mg, mo), f"{label}: mutations chr {c}"
        assert np.array_equal(g.download_haps(0, c), o.download_haps(0, c)), f"{label}: genotypes chr {c}"
    for x, y in zip(g.compute_ad(0), o.compute_ad(0)):
        assert helpers.bits_equal(x, y), f"{label}: A/D"


def _run(gpu_lib, oracle_lib, sc, path, second_generation=False):
    label = f"path {path}, {sc.name}"
    g = gpu_lib.create(1, sc.nchr, 1); o = oracle_lib.create(1, sc.nchr, 1)
    sc.apply(g); sc.apply(o, synth_packed)
    assert g.dbg_sampling_path() == 0
    sg, so = sc.reproduce(g), sc.reproduce(o)
    assert g.dbg_sampling_path() == path, f"{label}: ran sampling path {g.dbg_sampling_path()}"
    assert np.array_equal(sg, sc.sex), f"{label}: sexes against the stated chain"
    assert np.array_equal(sg, so), f"{label}: sexes"
    sc.check_designated(g, f"path {path},")
    _equal_to_oracle(g, o, sc, label)
    if second_generation:                   # the placed records as PARENTS: their pieces are what the next generation is cut from
        couples = np.array([(i, (i + 1) % sc.n_ind, 0, 1) for i in range(sc.n_ind)], dtype=np.int64)
        ms = None if sc.mut_seeds is None else sc.mut_seeds[::-1].copy()
        sg = g.reproduce(0, couples, sc.seed_reproduce + 1, ms); so = o.reproduce(0, couples, sc.seed_reproduce + 1, ms)
        assert g.dbg_sampling_path() == path and np.array_equal(sg, so), f"{label}: generation 2 sexes"
        _equal_to_oracle(g, o, sc, label + " generation 2")
    g.close(); o.close()


@pytest.mark.parametrize("group", ph.REPRODUCE_GROUPS)
@pytest.mark.parametrize("batched", [1, 0])
def test_placed_hits_with_a_mutation_map(gpu_lib, oracle_lib, monkeypatch, batched, group):
    """families A to E through k_sample_batched (default) and through k_mut_sample + k_rec_sample (GEV_SAMPLE_BATCHED=0)"""
    if batched:
        monkeypatch.delenv("GEV_SAMPLE_BATCHED", raising=False)
    else:
        monkeypatch.setenv("GEV_SAMPLE_BATCHED", "0")
    for sc in ph.reproduce_scenarios(group):
        _run(gpu_lib, oracle_lib, sc, BATCHED if batched else PER_TASK, second_generation=group in ("D", "E"))


@pytest.mark.parametrize("group", ph.CHAIN_GROUPS)
@pytest.mark.parametrize("wg", [None, "0"])
def test_placed_crossovers_in_the_serial_chain(gpu_lib, oracle_lib, monkeypatch, wg, group):
    """no mutation map: the crossover families with the designated gamete in task 0, through k_rec_chain_wg (GEV_CHAIN_WG unset) and
    k_rec_chain (GEV_CHAIN_WG=0)"""
    if wg is None:
        monkeypatch.delenv("GEV_CHAIN_WG", raising=False)
    else:
        monkeypatch.setenv("GEV_CHAIN_WG", wg)
    for sc in ph.chain_scenarios(group):
        _run(gpu_lib, oracle_lib, sc, CHAIN_WG if wg is None else CHAIN_WAVE, second_generation=group == "D")


@pytest.mark.parametrize("group", ph.GAMETE_GROUPS)
def test_placed_crossovers_in_one_gamete(gpu_lib, oracle_lib, group):
    """gev_dbg_sim_loc_rec (k_dbg_sim_loc_rec) with seeds in closed form: families A, B and C on the crossover scan with the exact
    high digit; it is no generation, so the context's sampling path stays 0"""
    g = gpu_lib.create(1, 1, 1)
    for name, rmap, seeds, _ in ph.gamete_cases(group):
        g.set_rmap(0, 0, *rmap)
        for seed, row, outcome in seeds:
            rows, bks, nxt = ph.predict_gamete(oracle_lib, rmap, seed)
            assert (row in rows) == (outcome == "hit")
            locs, nx = g.dbg_sim_loc_rec(0, 0, seed)
            assert [int(x) for x in locs] == bks and list(nx) == nxt, f"{name}: seed {seed}, row {row} stated {outcome}: {list(locs)} {nx}, stated {bks} {nxt}"
            ref, rnx = oracle_api.kat_sim_loc_rec(oracle_lib, rmap[0], rmap[1], rmap[2], seed)
            assert np.array_equal(locs, ref[1:-1]) and list(nx) == [int(rnx[0]), int(rnx[1])], f"{name}: seed {seed}"
    assert g.dbg_sampling_path() == 0
    g.close()
