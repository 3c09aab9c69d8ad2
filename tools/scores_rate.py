#!/usr/bin/env python3
"""Rate of gev_ind_scores (per-individual scores from the resident rows on the matrix cores, csrc/gev_indscore.h: G W with signed weight
columns) at BASELINE config 2's shape (100 000 individuals, 1 M SNPs), beside what stood in its place: the wsum of
gev_ind_genotype_counts, one unsigned weight vector per call; and one pca.components(k = 10) end to end.  Synthetic founders, one
generation, random weights over the whole +-2^30.

    python tools/scores_rate.py [n_ind] [n_loci] [--columns 4,16,64] [--repeats 5] [--k 10] [--out profiles/scores_rate.jsonl]

Every GPU step runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.  One JSON
line per step, printed and appended to --out:
  scores      one chromosome-wide gev_ind_scores call over all individuals, both outputs, host to host: median of --repeats after a
              warm-up; the same call over 256 SNPs (the fixed cost: the staging passes and the planes of every individual, the launches,
              the copies)
  yardstick   gev_ind_genotype_counts with one weight vector over the same ranges (the staging passes and one scalar walk per
              individual); its code is the parent commit's, untouched by this change.  The summary multiplies it by the number of columns
  pca         pca.components(k) over everybody, and how its time splits between the two device products (G W: gev_ind_scores, G^T Y:
              gev_snp_trait_sums) and the host (quantisation, mean terms, QR, the small eigenproblem)
No ratio is promised; no counter run is made here and the kernels are not timed apart."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = {"scores": 600, "yardstick": 600, "pca": 900}
FIXED_SNPS = 256


def population(n, L):
    from geneevolve_amd.capi import GevLibrary
    from geneevolve_amd.host import Simulation, SyntheticConfig
    cfg = SyntheticConfig(n, L, n_cv=1000, seed=12345)
    ctx = GevLibrary().create(1, 1, 1, 0)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 11); ctx.synth_cv_founders(0, 0, 0, 2 * n, 77)
    sim = Simulation(ctx, 1, 1, True)
    sim.ras_initial_human_gen0(0, n)
    sim.next_generation_rm(0, n)
    ctx.sync()
    return ctx


def median(times):
    return sorted(times)[len(times) // 2]


def timed(call, repeats):
    """seconds of `repeats` calls after one that does not count"""
    call()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return sorted(out)


def step_scores(args):
    import numpy as np
    n, L, S = args.n_ind, args.n_loci, args.n_scores
    ctx = population(n, L)
    w = np.random.RandomState(99).randint(-(1 << 30), (1 << 30) + 1, size=(S, L), dtype=np.int64).astype(np.int32)
    f = ctx.L._f("ind_scores")
    gscore = np.empty((S, n), dtype=np.int64); hetscore = np.empty((S, n), dtype=np.int64)
    few = np.ascontiguousarray(w[:, :min(FIXED_SNPS, L)])
    whole = timed(lambda: ctx.L.check(f(ctx.h, 0, 0, 0, L, 0, n, w, S, gscore, hetscore)), args.repeats)
    check = int(gscore[0, :1000].astype(object).sum())
    fixed = timed(lambda: ctx.L.check(f(ctx.h, 0, 0, 0, few.shape[1], 0, n, few, S, gscore, hetscore)), args.repeats)
    med = median(whole)
    rec = {"step": "scores", "n_ind": n, "n_loci": L, "n_scores": S, "repeats": args.repeats, "call_s": whole, "call_median_s": med,
           "fixed_snps": int(few.shape[1]), "fixed_call_s": fixed, "fixed_call_median_s": median(fixed), "genotype_weight_products_per_s": L * n * S / med,
           "plane_bytes": 2 * n * ((L + 63) // 64) * 8, "gscore_first_1000_sum": check}
    ctx.close()
    return rec


def step_yardstick(args):
    import numpy as np
    n, L = args.n_ind, args.n_loci
    ctx = population(n, L)
    w = np.random.RandomState(99).randint(0, (1 << 30) + 1, size=L, dtype=np.int64).astype(np.uint32)
    few = min(FIXED_SNPS, L)
    whole = timed(lambda: ctx.ind_genotype_counts(0, 0, 0, L, 0, n, weight=w), args.repeats)
    fixed = timed(lambda: ctx.ind_genotype_counts(0, 0, 0, few, 0, n, weight=w[:few]), args.repeats)
    rec = {"step": "yardstick", "n_ind": n, "n_loci": L, "repeats": args.repeats, "call_s": whole, "call_median_s": median(whole),
           "fixed_snps": few, "fixed_call_s": fixed, "fixed_call_median_s": median(fixed)}
    ctx.close()
    return rec


def step_pca(args):
    from geneevolve_amd import pca
    n, L = args.n_ind, args.n_loci
    ctx = population(n, L)
    spent = {"gw": 0.0, "gty": 0.0, "gw_calls": 0, "gty_calls": 0}

    def clocked(name, f):
        def g(*a):
            t0 = time.perf_counter()
            r = f(*a)
            spent[name] += time.perf_counter() - t0; spent[name + "_calls"] += 1
            return r
        return g
    gw, gty = pca._device_products(ctx)
    t0 = time.perf_counter()
    c = pca.components(ctx, 0, args.k, iters=args.iters, products=(clocked("gw", gw), clocked("gty", gty)))
    total = time.perf_counter() - t0
    rec = {"step": "pca", "n_ind": n, "n_loci": L, "k": args.k, "iters": args.iters, "columns": len(c.ritz), "polymorphic_snps": c.n_snps, "total_s": total,
           "ind_scores_s": spent["gw"], "ind_scores_calls": spent["gw_calls"], "snp_trait_sums_s": spent["gty"], "snp_trait_sums_calls": spent["gty_calls"],
           "host_s": total - spent["gw"] - spent["gty"], "values": [float(v) for v in c.values]}
    ctx.close()
    return rec


STEPS = {"scores": step_scores, "yardstick": step_yardstick, "pca": step_pca}


def run_step(args, step, extra, out):
    cmd = [sys.executable, os.path.abspath(__file__), str(args.n_ind), str(args.n_loci), "--repeats", str(args.repeats), "--k", str(args.k), "--iters", str(args.iters),
           "--step", step] + extra
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S[step])
        line = r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else json.dumps({"step": step, "args": extra, "error": f"exit status {r.returncode}"})
    except subprocess.TimeoutExpired:
        line = json.dumps({"step": step, "args": extra, "error": f"no result within {STEP_LIMIT_S[step]} s"})
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")
    rec = json.loads(line)
    return None if "error" in rec else rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_ind", nargs="?", type=int, default=100_000)
    ap.add_argument("n_loci", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--columns", default="4,16,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scores_rate.jsonl"))
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--n-scores", type=int)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(STEPS[args.step](args)), flush=True)
        return 0
    y = run_step(args, "yardstick", [], args.out)
    if not y:
        return 1                                                      # (nothing more is started on the device after a step that failed)
    for S in (int(v) for v in args.columns.split(",") if v):
        d = run_step(args, "scores", ["--n-scores", str(S)], args.out)
        if not d:
            return 1
        line = json.dumps({"summary": "scores_rate", "n_ind": args.n_ind, "n_loci": args.n_loci, "n_scores": S, "ind_scores_median_s": d["call_median_s"],
                           "ind_scores_fixed_median_s": d["fixed_call_median_s"], "wsum_one_vector_median_s": y["call_median_s"],
                           "wsum_times_columns_s": y["call_median_s"] * S, "wsum_route_over_ind_scores": y["call_median_s"] * S / d["call_median_s"]})
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if run_step(args, "pca", [], args.out) else 1


if __name__ == "__main__":
    sys.exit(main())
