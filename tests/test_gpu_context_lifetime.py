"""A context owns its streams, events and buffers, and gev_destroy releases them whatever the context was doing: contexts made and
closed in turn give the same generations bit for bit, a context may be closed with a generation pending and a head start queued, the
event that gev_generation_phenotypes creates on its first call goes with its context, a second close does nothing, and a gev_create
that fails hands out nothing.  The shapes are the smallest that run every stream: one population, one chromosome, 64 individuals,
300 SNPs, a mutation map (the batched sampling kernel) and the generation chain (a head start on the sampling stream)."""
import ctypes as C

import numpy as np
import pytest

from geneevolve_amd.capi import GevError
from geneevolve_amd.host import SyntheticConfig
from tests.helpers import bits_equal

pytestmark = pytest.mark.gpu

N, L, STATE0 = 64, 300, 123456789
CFG = SyntheticConfig(N, L, chrom_bp=1_000_000, map_step=5_000, rec_per_row=0.03, mut_per_row=0.02, n_cv=25, seed=61)
SCHEMES = [(0.5, 0.2, 0.0, 0.4, 0.3, 1.0)]                    # va, vd, vc, ve, vf, beta


def _context(gpu_lib, pedigree=False):
    g = gpu_lib.create(1, 1, 1)
    if pedigree:
        g.set_track_pedigree(True)
    CFG.apply_static(g)
    g.synth_founders(0, 0, 2 * N, 700)
    g.synth_cv_founders(0, 0, 0, 2 * N, 800)
    return g, g.init_gen0(0, N, 4242)


def _generations(g, n_gen=2):
    """n_gen generations through gev_generation_begin / _end with the chain's head start -> per generation what it returned and left
    on the device; the head start of the generation after the last is still queued when this returns"""
    g.set_generation_chain(0)
    out, state = [], STATE0
    for _ in range(n_gen):
        g.generation_begin(0, state, N)
        r = g.generation_end(want_couples=True)
        state = int(r["glob_state"])
        add, dom, _, _ = g.compute_ad(0, per_chr=False)
        parts, off = g.download_intervals(0, 0)
        out.append(dict(state=state, sex=r["sex"].copy(), couples=r["couples"].copy(), add=add, dom=dom, parts=parts, off=off))
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for gen, (x, y) in enumerate(zip(a, b), 1):
        assert x["state"] == y["state"], f"{what}: glob_state of generation {gen}"
        for k in ("sex", "couples", "parts", "off"):
            assert np.array_equal(x[k], y[k]), f"{what}: {k} of generation {gen}"
        assert bits_equal(x["add"], y["add"]) and bits_equal(x["dom"], y["dom"]), f"{what}: A/D of generation {gen}"


@pytest.fixture(scope="module")
def first_run(gpu_lib):
    """gen0 and two generations on the module's first context, which is closed with its last head start queued"""
    g, sex0 = _context(gpu_lib)
    gens = _generations(g)
    assert g.dbg_sampling_path() == 1, "the mutation map was meant to put the sampling on the batched kernel"
    g.close()
    assert len(gens[-1]["parts"]) > 2 * N and np.var(gens[-1]["add"]) > 0, "the shapes were meant to recombine and to carry A/D"
    return sex0, gens


def test_contexts_created_and_closed_in_turn_give_identical_generations(gpu_lib, first_run):
    """32 contexts in one process, one after the other: sexes, couples, A/D and interval lists of the last equal the first's"""
    sex0, gens = first_run
    for i in range(1, 32):
        g, s = _context(gpu_lib)
        got = _generations(g)
        g.close()
        assert np.array_equal(s, sex0), f"context {i}: sexes of generation 0"
    _same(got, gens, "context 32 against context 1")


def test_closing_with_a_generation_pending_and_a_head_start_queued(gpu_lib, first_run):
    """gev_destroy waits for every stream: a context is closed between gev_generation_begin and _end, the chain's head start of the
    generation after behind it; a fresh context on the same device then gives the first run's generations"""
    sex0, gens = first_run
    g, _ = _context(gpu_lib)
    done = _generations(g, 1)
    g.generation_begin(0, done[0]["state"], N)
    g.close()
    assert g.h is None
    g, s = _context(gpu_lib)
    got = _generations(g)
    g.close()
    assert np.array_equal(s, sex0)
    _same(got, gens, "after a close with work in flight")


def test_the_phenotype_event_goes_with_its_context(gpu_lib):
    """gev_generation_phenotypes creates its event on the first call: a context that made one closes, a second context's call gives
    the same result words (engine state, seeds, component variances) and phenotypes"""
    out = []
    for _ in range(2):
        g, _ = _context(gpu_lib, pedigree=True)
        g.generation_phenotypes(0, 0, 4242, SCHEMES)
        res = g.phenotypes_result(0)
        out.append((res, g.download_phenotypes(0, 0)))
        g.close()
    (ra, pa), (rb, pb) = out
    assert ra["glob_state"] == rb["glob_state"] and np.array_equal(ra["seeds"], rb["seeds"]) and bits_equal(ra["var"], rb["var"])
    assert ra["var"][0][6] > 0
    for k in pa:
        assert bits_equal(pa[k], pb[k]), k


def test_a_second_close_does_nothing_and_a_failed_create_hands_out_nothing(gpu_lib):
    import torch
    g, _ = _context(gpu_lib)
    g.close()
    assert g.h is None
    g.close()
    assert g.h is None
    ndev = torch.cuda.device_count()
    h = C.c_void_p(0xdead0)                                   # gev_create clears *out before anything can fail
    rc = gpu_lib._f("create")(C.byref(h), ndev, 1, 1, 1)      # one past the last device
    assert rc == -3 and h.value is None, f"GEV_EDEVICE and a null context expected: {rc}, {h.value}"
    assert "not present" in gpu_lib.last_error()
    with pytest.raises(GevError) as e:
        gpu_lib.create(1, 1, 1, device=ndev)
    assert e.value.code == -3
