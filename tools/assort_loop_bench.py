"""Generations/s of the closed loop with ASSORTATIVE mating (the reference's default mode), done two ways, at BASELINE config 2's
shape (100k individuals x 1M SNPs, one chromosome, one phenotype), logit 1 1 every generation, mat_cor 0.4, Poisson offspring
numbers.  Prints one JSON line.

  host   : gev_compute_selection with mating values and selection_value_func downloaded -> host.assort_mate (numpy / Python, ranks
           by gev_rank_f64) -> gev_reproduce with the couples uploaded -> gev_scale_ad_compute_gef
  device : gev_compute_selection with nothing downloaded -> gev_generation_begin_assort_selected / gev_generation_end (every
           ras_glob_seed() value drawn by the library, couples never leave it) -> gev_scale_ad_compute_gef
  split  : as device, but the generation as two calls: gev_assort_mate_selected, then gev_reproduce(couples = NULL)

Each mode gets a fresh context with the same inputs; --warmup generations first, then --steps timed ones.  `mate_ms_*` is the
mating step alone (host: download + assort_mate; split: the gev_assort_mate_selected call; not separable in device mode).
`couples_sha` hashes every generation's couples (device mode downloads them from gev_generation_end for this, after the clock
stops for the generation): equal hashes mean the modes formed the same couples."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def gef(ctx, sim, g, s2):
    """Simulation::ras_scale_AD_compute_GEF of phenotype 0 (va 0.4, ve 0.6, no D / F), nothing downloaded"""
    from geneevolve_amd.capi import gev_gef_params
    par = gev_gef_params(0.4, 0.0, 0.6, 0.0, 1.0, s2[0], s2[1], g, 0)
    seed = int(sim.ras_glob_seed()[0])
    ctx._call("scale_ad_compute_gef", C.c_int(0), C.c_int(0), C.byref(par), C.c_uint32(seed), None, None, None, None, None, None, None, None, None)


def run(mode, args):
    from geneevolve_amd.capi import GevLibrary
    from geneevolve_amd.host import Simulation, SyntheticConfig, assort_mate, comm_var
    lib = GevLibrary()
    cfg = SyntheticConfig(args.n_ind, args.n_loci, n_cv=args.n_cv, seed=12345)
    ctx = lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * args.n_ind, 1000)
    ctx.synth_cv_founders(0, 0, 0, 2 * args.n_ind, 2000)
    sim = Simulation(ctx, 4242, 1, True)
    sim.ras_initial_human_gen0(0, args.n_ind)
    ctx.reserve(0, int(args.n_ind * 1.05))                          # Poisson offspring numbers: the population size moves a little every generation
    add, dom, _, _ = ctx.compute_ad(0, per_chr=False)
    s2 = (comm_var(add[:, 0]), comm_var(dom[:, 0]))
    gef(ctx, sim, 0, s2)
    ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0], want=())
    times, mate_times, sizes = [], [], []
    h = hashlib.sha256()
    for g in range(1, args.warmup + args.steps + 1):
        t0 = time.perf_counter()
        if mode == "device":
            ctx.generation_begin_assort(0, sim.glob.x, args.n_ind, args.mat_cor, args.mm, False, "p", selected=True)
            r = ctx.generation_end(want_couples=False)
            sim.glob.x = int(r["glob_state"]); sim.sex[0] = r["sex"]
            gef(ctx, sim, g, s2)
            ctx.compute_selection(0, g, "logit", 1.0, 1.0, [1.0], [1.0], want=())
            t2 = time.perf_counter()
            times.append(t2 - t0); sizes.append(len(r["sex"]))
            h.update(ctx.last_assort_result(want_couples=True)[1].tobytes())
            continue
        seeds = [int(x) for x in sim.ras_glob_seed(4)]             # :2170, :2173, :2265, :2332
        if mode == "split":
            _, r = ctx.assort_mate_selected(0, seeds, args.n_ind, args.mat_cor, args.mm, False, "p", want_couples=False)
            n_off, couples = r["n_offspring"], None
        else:
            v = ctx.download_selection(0)
            n = len(v["mating_value"])
            couples = assort_mate(sim.sex[0], v["selection_value_func"], v["mating_value"], None, args.n_ind, args.mat_cor, seeds,
                                  args.mm, False, "p", rank=ctx.rank_f64)
            n_off = int(couples["num_offspring"][couples["inbreed"] == 0].sum())
            assert n == ctx.pop_size(0)
        t1 = time.perf_counter()
        rs = sim.ras_glob_seed(1 + n_off)
        sim.sex[0] = ctx.reproduce(0, couples, int(rs[0]), rs[1:], n_people=n_off)
        gef(ctx, sim, g, s2)
        ctx.compute_selection(0, g, "logit", 1.0, 1.0, [1.0], [1.0], want=())
        t2 = time.perf_counter()
        times.append(t2 - t0); mate_times.append(t1 - t0); sizes.append(n_off)
        h.update((couples if couples is not None else ctx.last_assort_result(want_couples=True)[1]).tobytes())
    ctx.sync()
    state = sim.glob.x
    ctx.close()
    t = np.array(times[args.warmup:])
    out = {"generations_per_s": round(float(len(t) / t.sum()), 2), "ms_per_generation_median": round(float(np.median(t)) * 1e3, 3)}
    if mate_times:
        m = np.array(mate_times[args.warmup:])
        out.update({"mate_ms_median": round(float(np.median(m)) * 1e3, 3), "mate_ms_min": round(float(m.min()) * 1e3, 3)})
    out.update({"offspring_last": int(sizes[-1]), "glob_state_after": int(state), "couples_sha": h.hexdigest()[:16]})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-ind", type=int, default=100_000)
    ap.add_argument("--n-loci", type=int, default=1_000_000)
    ap.add_argument("--n-cv", type=int, default=1000)
    ap.add_argument("--mat-cor", type=float, default=0.4)
    ap.add_argument("--mm", type=float, default=0.0)
    ap.add_argument("--modes", default="host,device,split")
    args = ap.parse_args()
    out = {"tool": "assort_loop_bench", "n_ind": args.n_ind, "n_loci": args.n_loci, "nphen": 1, "selection_function": "logit 1 1",
           "mat_cor": args.mat_cor, "mm_percent": args.mm, "offspring_dist": "p", "steps": args.steps, "warmup": args.warmup}
    for mode in args.modes.split(","):
        out[mode] = run(mode, args)
    if "host" in out and "device" in out:
        out["device_over_host"] = round(out["device"]["generations_per_s"] / out["host"]["generations_per_s"], 3)
        out["same_couples"] = len({out[m]["couples_sha"] for m in out if isinstance(out[m], dict)}) == 1
    print(json.dumps(out))


if __name__ == "__main__":
    main()
