"""A head start is only a schedule: whatever sits in a scratch set when a generation begins -- nothing, gev_presample's sampling
(matching or not), the generation chain's, or either of them dropped by a redo of the generation in flight -- every begin call
(gev_reproduce_begin with host couples or behind gev_random_mate, gev_generation_begin, gev_generation_begin_assort) must give
the generation that a twin context gives which was driven through the same calls without the head start.  Both overlap modes.
The test pins results only; which stream waits for what in each case is the library's business (take_head_start)."""
import numpy as np
import pytest

from geneevolve_amd.host import GlobSeedStream, SyntheticConfig, synthetic_random_mate
from tests import helpers

pytestmark = pytest.mark.gpu

N, NCHR = 1000, 2
CFG = SyntheticConfig(N, 1500, nchr=NCHR, chrom_bp=1_000_000, map_step=5_000, rec_per_row=0.03, mut_per_row=0.02, n_cv=25, seed=53)
LEFT = ("nothing", "presample", "presample_other_seed", "presample_with_mut_seeds", "chain", "presample_dropped", "chain_dropped")
BEGIN = ("reproduce_host_couples", "reproduce_after_random_mate", "generation", "generation_assort")


def _context(gpu_lib, overlap):
    g = gpu_lib.create(1, NCHR, 1)
    g.set_overlap(overlap)
    CFG.apply_static(g)
    for c in range(NCHR):
        g.synth_founders(0, c, 2 * N, 700 + c)
        g.synth_cv_founders(0, 0, c, 2 * N, 800 + c)
    return g, g.init_gen0(0, N, 4242)


def _drive(gpu_lib, overlap, left, begin, head_start):
    """generation 1 with `left` queued behind it (head_start = False: the same calls without it), then generation 2 through
    `begin` -> what generation 2 returned and left on the device"""
    g, sex0 = _context(gpu_lib, overlap)
    glob = GlobSeedStream(77)
    seeds1, seeds2 = glob.draw(1 + N * NCHR), glob.draw(1 + N * NCHR)
    # the begin under test has no mutation seeds of its own in one case: only gev_reproduce_begin can say so
    mut2 = None if left == "presample_with_mut_seeds" and begin.startswith("reproduce") else seeds2[1:]
    if left.startswith("chain"):
        if head_start:
            g.set_generation_chain(0)
        g.generation_begin(0, 123456789, N)
        r1 = g.generation_end(want_couples=False)
        sex1, state2 = r1["sex"], int(r1["glob_state"])     # (no draws in between: the state the head start assumed)
        # (that the chain head start is really taken with this state is what test_head_start_across_generations_is_only_a_schedule
        # pins; were it not, this cell would quietly become one more mismatch case)
    else:
        g.reproduce_begin(0, synthetic_random_mate(sex0, N, np.random.default_rng(1)), int(seeds1[0]), seeds1[1:], n_people=N)
        if head_start and left.startswith("presample"):
            g.presample(0, int(seeds2[0]) + (left == "presample_other_seed"), seeds2[1:], N)
        sex1, state2 = g.reproduce_end(), 987654321
    if left.endswith("dropped"):
        assert g.redo_count() > 0, "the tiny overflow regions were meant to have generation 1 enqueued again"
    out = {}
    if begin == "reproduce_host_couples":
        g.reproduce_begin(0, synthetic_random_mate(sex1, N, np.random.default_rng(2)), int(seeds2[0]), mut2, n_people=N)
        out["sex"] = g.reproduce_end()
    elif begin == "reproduce_after_random_mate":
        out["couples"], out["num_males_mate"], out["num_females_mate"] = g.random_mate(0, 31337, None, N)
        out["sex"] = g.reproduce(0, None, int(seeds2[0]), mut2, n_people=N)      # (gev_reproduce_begin and _end in one call)
    else:
        if begin == "generation":
            g.generation_begin(0, state2, N)
        else:
            g.generation_begin_assort(0, state2, N, 0.4, offspring_dist="f", mating_value=np.sin(np.arange(N, dtype=np.float64)))
        out.update(g.generation_end(want_couples=True))
    out["ad"] = g.compute_ad(0)
    for c in range(NCHR):
        out[f"intervals{c}"] = g.download_intervals(0, c)
        out[f"mutations{c}"] = g.download_mutations(0, c)
    g.close()
    return out


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("begin", BEGIN)
@pytest.mark.parametrize("left", LEFT)
def test_a_begin_call_gives_the_same_generation_whatever_head_start_it_finds(gpu_lib, monkeypatch, left, begin, overlap):
    if left.endswith("dropped"):
        monkeypatch.setenv("GEV_OVF_CAP", "8")               # read when a context is created
    a = _drive(gpu_lib, overlap, left, begin, head_start=True)
    b = _drive(gpu_lib, overlap, left, begin, head_start=False)
    assert a.keys() == b.keys()
    for k in a:
        if k == "ad":
            assert all(helpers.bits_equal(x, y) for x, y in zip(a[k], b[k])), "A/D"
        elif isinstance(a[k], tuple):
            assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])
    assert len(a["sex"]) == N and len(a["mutations0"][0]) > 0 and np.var(a["ad"][0]) > 0
