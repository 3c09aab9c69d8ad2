#!/usr/bin/env python3
"""SHA-256 of the raw output bytes of every call that draws normal values or sums a mean / variance on the device (csrc/gev_normal.h):
gev_scale_ad_compute_gef, gev_compute_selection, gev_generation_phenotypes and gev_assort_mate.  Two builds of the library compute
the same thing exactly when their outputs here are identical line for line; GEV_LIBRARY_PATH selects the build.

    GEV_LIBRARY_PATH=/path/to/libgeneevolve_amd.so python tools/normal_paths_digest.py > digest.jsonl

Synthetic inputs only.  One JSON line per case:
  gef        generation 0 (noise and parental streams) and generation 1 (parents' effects and a family effect from the host) at sizes
             around the edges of the candidate blocks and of the sums, six output vectors each
  selection  generation-0 statistics, then the three value vectors of all six selection functions at generation 1
  phenotypes a two-phenotype step with vc > 0 at generations 0 and 1 (one generation of random mating in between): seeds, variances
             and the seven component planes
  assort     couples and result of gev_assort_mate, 'p' and 'f' offspring numbers, with and without avoid_inbreeding"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GEF_SIZES = [1, 2, 3, 2866, 2867, 100_003, 1_000_001]
GEF_OUTPUTS = ("additive", "dominance", "bv", "e_noise", "parental_effect", "phen")
FUNCS = [("", 0.0, 0.0), ("logit", 1.0, 1.0), ("probit", -0.3, 0.8), ("stab", 0.2, 1.3), ("thr", 0.4, 0.1), ("none", 0.0, 0.0)]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def emit(case, **kw):
    print(json.dumps(dict(case=case, **kw)), flush=True)


def population(lib, n, nphen, track=False):
    """one population of n whose raw A/D come from the host (nothing depends on genotypes)"""
    from geneevolve_amd.host import SyntheticConfig
    cfg = SyntheticConfig(max(n, 2), 256, chrom_bp=2_000_000, map_step=10_000, n_cv=16, nphen=nphen, seed=3)
    ctx = lib.create(1, 1, nphen)
    if track:
        ctx.set_track_pedigree(True)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 5)
    for p in range(nphen):
        ctx.synth_cv_founders(0, p, 0, 2 * n, 13 + p)
    sex = ctx.init_gen0(0, n, 780)
    rng = np.random.default_rng(n)
    ctx.set_ad(0, rng.standard_normal((n, nphen)), rng.standard_normal((n, nphen)))
    return ctx, sex, rng


def case_gef(lib):
    for n in GEF_SIZES:
        ctx, _, rng = population(lib, n, 1)
        cs, ff, fm = rng.standard_normal(n) * 0.3, rng.standard_normal(n), rng.standard_normal(n)
        g0 = ctx.scale_ad_compute_gef(0, 0, 0, 1000 + n, 0.5, 0.2, 0.4, 0.3, 0.7, 1.7, 0.3)
        emit("gef", n=n, gen=0, sha256=sha(*[g0[k] for k in GEF_OUTPUTS]))
        g1 = ctx.scale_ad_compute_gef(0, 0, 1, 2000 + n, 0.5, 0.2, 0.4, 0.3, 0.7, 1.7, 0.3, common_sibling=cs, f_father=ff, f_mother=fm)
        emit("gef", n=n, gen=1, sha256=sha(*[g1[k] for k in GEF_OUTPUTS]))
        if n == 100_003:
            case_selection(ctx, n)
        ctx.close()


def case_selection(ctx, n):
    """on the phenotypes the generation-1 call above has left in the library"""
    names = ("mating_value", "selection_value", "selection_value_func")
    v = ctx.compute_selection(0, 0, "none", 0, 0, [0.8], [1.0], phen_shift=[0.25])
    emit("selection", n=n, gen=0, func="none", gen0_mean_var=sha(np.array(ctx.get_selection_gen0(0))), sha256=sha(*[v[k] for k in names]))
    for kind, p1, p2 in FUNCS:
        v = ctx.compute_selection(0, 1, kind, p1, p2, [0.8], [1.0], phen_shift=[0.25])
        emit("selection", n=n, gen=1, func=kind, sha256=sha(*[v[k] for k in names]))


def case_phenotypes(lib, n=2_000):
    from geneevolve_amd.capi import PHENOTYPE_COMPONENTS
    from geneevolve_amd.host import Simulation, SyntheticConfig
    cfg = SyntheticConfig(n, 2048, chrom_bp=4_000_000, map_step=20_000, rec_per_row=1e-3, mut_per_row=1e-4, n_cv=100, nphen=2, seed=6, vd=0.2)
    ctx = lib.create(1, 1, 2)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 51)
    for p in range(2):
        ctx.synth_cv_founders(0, p, 0, 2 * n, 52 + p)
    sim = Simulation(ctx, 4242, 1, True, device_pedigree=True)
    sim.ras_initial_human_gen0(0, n)
    schemes = [(0.5, 0.1, 0.1, 0.2, 0.1, 1.0), (0.4, 0.0, 0.2, 0.3, 0.1, 0.9)]         # va, vd, vc, ve, vf, beta
    for g in (0, 1):
        if g:
            sim.next_generation_rm_selected(0, n)
        sim.generation_phenotypes(0, g, schemes, 1)
        r = sim.phenotypes_result(0)
        comps = [ctx.download_phenotypes(0, p) for p in range(2)]
        emit("phenotypes", n=n, gen=g, seeds=[int(s) for s in r["seeds"]], var=sha(r["var"]),
             sha256=sha(*[c[k] for c in comps for k in PHENOTYPE_COMPONENTS]))
        ctx.compute_selection(0, g, "logit", 0.2, 0.8, [1.0, 0.5], [1.0, 1.0], want=())
        sim.save_prev_gen(0)
    ctx.close()


def case_assort(lib):
    for n in (2_000, 100_000):
        ctx, _, rng = population(lib, n, 1)
        mv = rng.standard_normal(n)
        ped = rng.integers(0, max(n // 4, 1), size=(n, 5))
        for avoid in (False, True):
            size = n
            for dist in ("p", "f"):
                couples, res = ctx.assort_mate(0, [11, 22, 33, 44], mv, None, size, 0.4, 0.0, avoid, dist, ped if avoid else None)
                emit("assort", n=n, pop_size=size, offspring_dist=dist, avoid_inbreeding=avoid, result=res, sha256=sha(couples))
                if avoid:                                   # 'f' with avoid_inbreeding: the couples that may breed must divide the size
                    size = 2 * (res["n_couples"] - res["n_inbreed"])
        ctx.close()


def main():
    from geneevolve_amd.capi import GevLibrary
    lib = GevLibrary()
    case_gef(lib)
    case_phenotypes(lib)
    case_assort(lib)


if __name__ == "__main__":
    main()
