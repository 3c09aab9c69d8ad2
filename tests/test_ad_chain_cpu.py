"""The oracle alone satisfies what the cases of tests/test_gpu_ad_chain.py state about themselves (tests/ad_chain.py): new mutations
land on CV positions and move the allele counts in every generation, some task hits one position twice on the same haplotype and
the second hit changes nothing, and a CV behind the chromosome's end contributes nothing.  No GPU."""
import numpy as np
import pytest

from tests import ad_chain as ac
from tests import helpers


def _generations(oracle_lib, case, gens):
    o = oracle_lib.create(1, case.nchr, case.nphen)
    case.apply(o)
    o.init_gen0(0, case.n_ind, 77)
    out = []
    for gen in range(1, gens + 1):
        o.reproduce(0, case.couples(), 500 + gen, case.mut_seeds(gen) if case.with_mut else None)
        ad = o.compute_ad(0)
        out.append(dict(ad=ad, frq=o.get_cv_freq(0, 0, 0), cv=o.download_cv(0, 0, 0), muts=o.download_mutations(0, 0), parts=o.download_intervals(0, 0)))
    o.close()
    return out


def _bit(w, row, j):
    return (int(w[row, j // 64]) >> (j % 64)) & 1


@pytest.mark.parametrize("ncv", [1, 128])
def test_new_mutations_land_on_cv_positions_and_repeat(oracle_lib, ncv):
    case = ac.Case(130, ncv)
    hot = ac.hot_positions(case.cv[0][0][0])
    col = {int(x): j for j, x in enumerate(case.cv[0][0][0])}
    gens = _generations(oracle_lib, case, 3)
    for gen in (1, 2, 3):
        hits = case.predicted_hits(oracle_lib, gen)
        assert sum(len(h) for h in hits.values()) >= case.n_ind, "nearly every task was meant to hit a CV position"
        assert ac.repeated_hits(hits), f"generation {gen}: no task hits one position twice on the same haplotype"
        muts, moff = gens[gen - 1]["muts"]
        for t, hs in hits.items():          # the placed hits are in the offspring's lists (one chromosome: task == individual)
            for x, side in hs:
                row = 2 * t + side
                assert x in [int(v) for v in muts[int(moff[row]):int(moff[row + 1])]], (gen, t, x, side)
        if gen > 1:                         # the allele counts of the hot columns move in every generation
            assert all(gens[gen - 1]["frq"][col[x]] != gens[gen - 2]["frq"][col[x]] for x in hot), gen
    # generation 1, where every inherited list is empty: the resolved allele of a hot column is the founder's, flipped ONCE where the
    # position is in the row's list -- however often it was hit (a set)
    founders = ac.synth_packed(31, 2 * case.n_ind, ncv)
    (muts, moff), (parts, poff), cv = gens[0]["muts"], gens[0]["parts"], gens[0]["cv"]
    hits = case.predicted_hits(oracle_lib, 1)
    twice = {(2 * t + s, x) for t, x, s in ac.repeated_hits(hits)}
    flipped = 0
    for row in range(2 * case.n_ind):
        mine = {int(v) for v in muts[int(moff[row]):int(moff[row + 1])]}
        for x in hot:
            src = [int(p["hap_index"]) for p in parts[int(poff[row]):int(poff[row + 1])] if int(p["st"]) <= x < int(p["en"])]
            assert len(src) == 1
            assert _bit(cv, row, col[x]) == _bit(founders, src[0], col[x]) ^ (x in mine), (row, x)
            flipped += x in mine
            assert (row, x) not in twice or x in mine
    assert flipped >= case.n_ind


def test_a_cv_behind_the_chromosome_end_contributes_nothing(oracle_lib):
    case = ac.Case(130, 128, vd=(0.5,), uncovered=True)
    pos, a, d, vd = case.cv[0][0]
    assert not (ac.BP0 <= int(pos[-1]) < ac.BP_END) and all(ac.BP0 <= int(x) < ac.BP_END for x in pos[:-1])
    assert a[-1] != 0 and d[-1] != 0
    zeroed = ac.Case(130, 128, vd=(0.5,), uncovered=True)
    zeroed.cv[0][0] = (pos, np.r_[a[:-1], 0.0], np.r_[d[:-1], 0.0], vd)
    for x, y in zip(_generations(oracle_lib, case, 2), _generations(oracle_lib, zeroed, 2)):
        assert all(helpers.bits_equal(p, q) for p, q in zip(x["ad"], y["ad"]))
        assert np.array_equal(x["frq"], y["frq"]) and x["frq"][-1] == 0 and 0 < x["frq"][-2] < 1     # (no part holds it: its alleles stay unresolved)
