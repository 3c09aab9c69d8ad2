"""Generations/s of the closed loop WITH a selection function, done two ways, at BASELINE config 2's shape (100k individuals x 1M
SNPs, one chromosome, one phenotype, logit 1 1 every generation).  Prints one JSON line.

  host   : gev_generation_begin(host svf) / _end -> gev_scale_ad_compute_gef with the phenotype downloaded -> the host forms mating
           and selection values, standardises them to generation 0 and applies logit (numpy, the reference's formula) -> the svf
           array goes back up with the next gev_generation_begin
  device : gev_generation_begin_selected / _end -> gev_scale_ad_compute_gef with no output downloaded -> gev_compute_selection with
           no output (only enqueued) -> the next gev_generation_begin_selected

Both run with the head start across generations on (gev_set_generation_chain(1): one ras_glob_seed() per phenotype for the GEF,
src/Simulation.cpp:3078) unless --no-chain.  Each mode gets a fresh context with the same inputs; --warmup generations first, then
--steps timed ones."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def gef(ctx, sim, g, s2, want_phen):
    """Simulation::ras_scale_AD_compute_GEF of phenotype 0 (va 0.4, ve 0.6, no D / F); downloads the phenotype only when asked"""
    from geneevolve_amd.capi import gev_gef_params
    n = ctx.pop_size(0)
    par = gev_gef_params(0.4, 0.0, 0.6, 0.0, 1.0, s2[0], s2[1], g, 0)
    phen = np.zeros(n) if want_phen else None
    seed = int(sim.ras_glob_seed()[0])
    ptr = phen.ctypes.data_as(C.c_void_p) if want_phen else None
    ctx._call("scale_ad_compute_gef", C.c_int(0), C.c_int(0), C.byref(par), C.c_uint32(seed), None, None, None, None, None, None, None, None, ptr)
    return phen


def run(mode, args):
    from geneevolve_amd.capi import GevLibrary
    from geneevolve_amd.host import Simulation, SyntheticConfig, comm_mean, comm_var
    lib = GevLibrary()
    cfg = SyntheticConfig(args.n_ind, args.n_loci, n_cv=args.n_cv, seed=12345)
    ctx = lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * args.n_ind, 1000)
    ctx.synth_cv_founders(0, 0, 0, 2 * args.n_ind, 2000)
    if not args.no_chain:
        ctx.set_generation_chain(1)
    sim = Simulation(ctx, 4242, 1, True)
    sim.ras_initial_human_gen0(0, args.n_ind)
    add, dom, _, _ = ctx.compute_ad(0, per_chr=False)
    s2 = (comm_var(add[:, 0]), comm_var(dom[:, 0]))
    b0, b1 = 1.0, 1.0
    phen = gef(ctx, sim, 0, s2, True)
    sv0 = (comm_mean(phen), comm_var(phen))                         # generation-0 standardisation (:3326-3330), host side
    if mode == "device":
        ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0], want=())
    svf = np.ones(args.n_ind)
    times = []
    for g in range(1, args.warmup + args.steps + 1):
        t0 = time.perf_counter()
        if mode == "device":
            sim.next_generation_rm_selected(0, args.n_ind)
            gef(ctx, sim, g, s2, False)
            ctx.compute_selection(0, g, "logit", b0, b1, [1.0], [1.0], want=())
        else:
            sim.next_generation_rm(0, args.n_ind, svf)
            phen = gef(ctx, sim, g, s2, True)
            mv = 0.0 + 1.0 * phen; sv = 0.0 + 1.0 * phen             # (:3310-3318; mv is what assortative mating would read)
            z = (sv - sv0[0]) / np.sqrt(sv0[1]) if sv0[1] > 0 else sv - sv0[0]
            with np.errstate(over="ignore", invalid="ignore"):
                y = np.exp(b0 + b1 * z)
                svf = y / (1 + y)
        times.append(time.perf_counter() - t0)
    ctx.sync()
    state = sim.glob.x
    ctx.close()
    t = np.array(times[args.warmup:])
    return {"generations_per_s": round(float(len(t) / t.sum()), 2), "ms_per_generation_median": round(float(np.median(t)) * 1e3, 3),
            "ms_per_generation_min": round(float(t.min()) * 1e3, 3), "glob_state_after": int(state)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-ind", type=int, default=100_000)
    ap.add_argument("--n-loci", type=int, default=1_000_000)
    ap.add_argument("--n-cv", type=int, default=1000)
    ap.add_argument("--no-chain", action="store_true", help="no head start across generations")
    ap.add_argument("--modes", default="host,device")
    args = ap.parse_args()
    out = {"tool": "selection_loop_bench", "n_ind": args.n_ind, "n_loci": args.n_loci, "nphen": 1, "selection_function": "logit 1 1",
           "head_start": not args.no_chain, "steps": args.steps, "warmup": args.warmup}
    for mode in args.modes.split(","):
        out[mode] = run(mode, args)
    if "host" in out and "device" in out:
        out["device_over_host"] = round(out["device"]["generations_per_s"] / out["host"]["generations_per_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
