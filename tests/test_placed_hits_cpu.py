"""The placed-hit constructions of tests/placed_hits.py against the oracle alone: every case is built, run through the oracle
(reproduce, download_intervals, download_mutations) and must show the stated expectation on its designated tasks, so the GPU file
compares the kernels with claims the reference itself satisfies.

Cases (none left out):
  A  draw edges          48 reproduce scenarios (12 scan lengths x hit / miss x cold / warm; 49 crossover + 50 mutation edges each
                         way), 196 serial-chain scenarios (task 0), 44 maps / 196 gametes for gev_dbg_sim_loc_rec
  B  threshold digit     the window claim a_lo <= a < a_hi on every placed probability of family A; the b1 branch: a miss as a
                         mutation task and as a gamete (a hit on b1 cannot be built: no engine state reaches it, see
                         test_b1_branch_windows_and_why_only_the_miss_side_exists)
  C  prefilter edge      5 points (mutation tasks and gametes), all-candidates maps hit / miss
  D  count edges         10 reproduce scenarios (k_pat 6 7 8 9, k_mat 7 8, n_mut 6 7 8 9), 6 serial-chain scenarios
  E  place in the batch  8 scenarios (17, 18, 33, 18 tasks x gamete / mutation), tasks 0 1 7 8 9 last
search_seed: 416 searches, largest trial count seen 1563 of 50 000 allowed."""
import numpy as np
import pytest

from oracle import oracle_api
from tests import placed_hits as ph
from tests.synth import synth_packed


def test_arithmetic_the_constructions_rest_on(oracle_lib):
    ol = oracle_lib
    for E in (0, 1, 2, 12345, ph.M31 - 1, ph.M31, ph.M31 + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1):
        out = oracle_api.kat_minstd(ol, E & 0xFFFFFFFF, 12)
        u = oracle_api.kat_u01(ol, E & 0xFFFFFFFF, 6)
        for d in range(6):
            a, b = ph.digits(E, d)
            assert (b + 1, a + 1) == (int(out[2 * d]), int(out[2 * d + 1])), (E, d)
            assert ph.canonical(ol, a, b) == u[d]
        assert [int(x) for x in ph.high_digits(E, 6)] == [ph.digits(E, d)[0] for d in range(6)]
    for d in (0, 63, 64, 2047, 2048, 2049):
        for wrap in (False, True):
            for off in (1, 2):
                s = ph.solve_seed(d, 777_777 + d, off, wrap)
                assert (s >= 2 ** 31) == wrap and ph.digits(s + off, d)[0] == 777_777 + d


def test_straddle_decides_the_draw_in_the_reference(oracle_lib):
    """p_hit = nextafter(r, 1) makes draw d a crossover of kat_sim_loc_rec, p_miss = r does not, at the six draw indices either side
    of the scan's block steps; the restated gamete agrees with the reference call"""
    ol = oracle_lib
    bp, prob, dist = ph.rmap_rows(2100)
    for d in (0, 63, 64, 2047, 2048, 2049):
        seed = ph.solve_seed(d, 900_000 + d, 1)
        for p, want in zip(ph.straddle(ph.draw_value(ol, seed + 1, d)), (True, False)):
            pr = prob.copy(); pr[d] = p
            locs, nx = oracle_api.kat_sim_loc_rec(ol, bp, pr, dist, seed)
            assert (len(locs) == 3) == want and len(locs) == (3 if want else 2), (d, p)
            rows, bks, nxt = ph.predict_gamete(ol, (bp, pr, dist), seed)
            assert rows == ([d] if want else []) and [int(x) for x in locs[1:-1]] == bks and [int(nx[0]), int(nx[1])] == nxt


def _run_on_oracle(ol, sc):
    o = ol.create(1, sc.nchr, 1)
    sc.apply(o, synth_packed)
    sex = sc.reproduce(o)
    assert np.array_equal(sex, sc.sex), f"{sc.name}: sexes"
    sc.check_designated(o, "oracle")
    o.close()


def _check_windows(gl, windows, name):
    for p, a in windows:
        a_lo, a_hi, _, _ = ph.threshold(gl, p)
        assert a_lo <= a < a_hi, f"{name}: p = {p!r}: a = {a} is outside the window [{a_lo}, {a_hi}): the low digit would not decide"


@pytest.mark.parametrize("group", ph.REPRODUCE_GROUPS)
def test_reproduce_scenarios_hold_on_the_oracle(gpu_lib, oracle_lib, group):
    scs = ph.reproduce_scenarios(group)
    assert len(scs) == {"A": 4, "B": 4, "D": 10, "E": 8}[group[0]]
    for sc in scs:
        assert sc.designated and len(sc.claims) >= len({t for t, _, _ in sc.designated})
        _run_on_oracle(oracle_lib, sc)
        if group[0] == "A":
            n = int(group[1:])
            assert len(sc.windows) == len(ph.edge_draws(n)) * (2 if n >= 2 else 1)
            _check_windows(gpu_lib, sc.windows, sc.name)
    if group == "BC":
        _check_windows(gpu_lib, scs[0].windows, scs[0].name)


@pytest.mark.parametrize("group", ph.CHAIN_GROUPS)
def test_chain_scenarios_hold_on_the_oracle(gpu_lib, oracle_lib, group):
    scs = ph.chain_scenarios(group)
    assert len(scs) == (4 * len(ph.edge_draws(int(group[1:]))) if group[0] == "A" else 6)
    for sc in scs:
        assert sc.mmaps is None and sc.designated and all(t == 0 for t, _, _ in sc.designated)
        _run_on_oracle(oracle_lib, sc)
        if group[0] == "A":
            _check_windows(gpu_lib, sc.windows, sc.name)


@pytest.mark.parametrize("group", ph.GAMETE_GROUPS)
def test_gamete_cases_hold_on_the_oracle(gpu_lib, oracle_lib, group):
    cases = ph.gamete_cases(group)
    assert len(cases) == (4 if group[0] == "A" else 4)
    for name, rmap, seeds, windows in cases:
        if group[0] == "A":
            assert len(seeds) == len(windows) == len(ph.edge_draws(int(group[1:])))
        _check_windows(gpu_lib, windows, name)
        for seed, row, outcome in seeds:
            rows, bks, nxt = ph.predict_gamete(oracle_lib, rmap, seed)
            assert (row in rows) == (outcome == "hit"), f"{name}: seed {seed} row {row}: stated {outcome}, rows {rows}"
            locs, nx = oracle_api.kat_sim_loc_rec(oracle_lib, rmap[0], rmap[1], rmap[2], seed)
            assert [int(x) for x in locs[1:-1]] == bks and [int(nx[0]), int(nx[1])] == nxt, f"{name}: seed {seed}"


def test_b1_branch_windows_and_why_only_the_miss_side_exists(gpu_lib, oracle_lib):
    """the issue asks for one hit and one miss on the second digit of a two-wide window.  Two-wide windows exist (the walk finds
    them), and a = a_lo + 1 can be placed, but the engine's own low digit at that a is always on the miss side: see
    placed_hits.b1_probabilities.  Asserted here for every window of the list: b1 is tiny, b is not"""
    found, windows = ph.b1_probabilities(gpu_lib, oracle_lib)
    assert "miss" in found and len(windows) >= 20
    for p, a_lo, a_hi, b0, b1, b in windows:
        assert a_hi - a_lo == 2 and 0 < b1 <= 64 and b >= b1 and b0 > b1
        assert ph.canonical(oracle_lib, a_lo + 1, b1 - 1) < p <= ph.canonical(oracle_lib, a_lo + 1, b1)      # b1 is what decides at a_lo + 1
        assert ph.canonical(oracle_lib, a_lo + 1, b) >= p
    assert "hit" not in found
    p, a, seed = found["miss"]
    assert ph.threshold(gpu_lib, p)[0] + 1 == a


def test_every_seed_search_stayed_under_its_cap(oracle_lib):
    for g in ph.REPRODUCE_GROUPS:
        ph.reproduce_scenarios(g)
    for g in ph.CHAIN_GROUPS:
        ph.chain_scenarios(g)
    n_searched = 49 * 4 + 196 + 4 * 6            # family A (crossover edges), A on task 0, E gamete scenarios
    assert len(ph.search_trials) == n_searched and max(ph.search_trials) < ph.SEARCH_CAP
    print(f"search_seed: {len(ph.search_trials)} searches, largest trial count {max(ph.search_trials)}")
