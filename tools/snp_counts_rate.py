#!/usr/bin/env python3
"""Rate of gev_snp_genotype_counts (per-SNP heterozygous / homozygous-alt counts from the resident rows, csrc/gev_snpcount.h) at
BASELINE config 2's shape, beside the only other route to the same numbers: gev_download_snp_major over the same SNPs plus a host
popcount.  Synthetic founders, one generation.

    python tools/snp_counts_rate.py [n_ind] [n_loci] [--repeats 5] [--route-repeats 1] [--route-chunk 32768]

Every GPU step runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.  One JSON
line per step, then one summary line:
  counts     one chromosome-wide call, host to host (the call returns with both vectors in host memory): median of --repeats after a
             warm-up; rows x row bytes over that time as a fraction of 8 TB/s; the same call over ONE individual (the memset and the
             copy-out of the two vectors, with next to nothing to read) as the call's fixed cost
  snp_major  the whole SNP range through gev_download_snp_major in runs of --route-chunk SNPs into one reused host buffer, each run
             popcounted on the host (numpy bitwise_count on the pair masks); download and popcount times apart
The two steps build the same population from the same seeds; the summary says whether their counts agree (SHA-256)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_SPEC = 8.0e12
STEP_LIMIT_S = {"counts": 420, "snp_major": 900}


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


def digest(het, hom):
    return hashlib.sha256(het.tobytes() + hom.tobytes()).hexdigest()


def step_counts(args):
    import numpy as np
    from geneevolve_amd import capi
    n, L = args.n_ind, args.n_loci
    ctx = population(n, L)
    het, hom = np.empty(L, dtype=np.uint32), np.empty(L, dtype=np.uint32)
    f = ctx.L._f("snp_genotype_counts")

    def call(n_ind):
        t0 = time.perf_counter()
        ctx.L.check(f(ctx.h, 0, 0, 0, L, 0, n_ind, het, hom))
        return time.perf_counter() - t0
    call(1); call(n)                                                  # warm-up: the CSR lists, the count vectors, the code objects
    fixed = sorted(call(1) for _ in range(args.repeats))
    times = sorted(call(n) for _ in range(args.repeats))
    med = times[len(times) // 2]
    row_bytes = (L + 127) // 128 * 16                                 # the 16-byte chunks of a row that hold a SNP
    nbytes = 2 * n * row_bytes
    muts, _ = ctx.download_mutations(0, 0)
    rec = {"step": "counts", "n_ind": n, "n_loci": L, "repeats": args.repeats, "call_s": times, "call_median_s": med,
           "fixed_cost_s": fixed, "fixed_cost_median_s": fixed[len(fixed) // 2], "bytes_read": nbytes, "bytes_per_s": nbytes / med,
           "fraction_of_8TBps": nbytes / med / HBM_SPEC, "floor_at_8TBps_s": nbytes / HBM_SPEC, "mutations": int(len(muts)),
           "alt_alleles": int(het.sum(dtype=np.int64) + 2 * hom.sum(dtype=np.int64)), "sha256": digest(het, hom)}
    ctx.close()
    print(json.dumps(rec), flush=True)


def step_snp_major(args):
    import numpy as np
    from geneevolve_amd import capi
    n, L = args.n_ind, args.n_loci
    ctx = population(n, L)
    w = capi.words_for(2 * n)
    chunk = min(args.route_chunk, L)
    buf = np.empty((chunk, w), dtype=np.uint64)
    het, hom = np.empty(L, dtype=np.uint32), np.empty(L, dtype=np.uint32)
    pairs = np.uint64(0x5555555555555555)
    f = ctx.L._f("download_snp_major")

    def run(s0, ns):
        t0 = time.perf_counter()
        ctx.L.check(f(ctx.h, 0, 0, s0, ns, buf, w))
        t1 = time.perf_counter()
        b = buf[:ns]
        sh = b >> np.uint64(1)                                         # haplotypes 2i and 2i+1 are bits 2i and 2i+1 of a SNP's row
        het[s0:s0 + ns] = np.bitwise_count((b ^ sh) & pairs).sum(axis=1, dtype=np.uint32)
        hom[s0:s0 + ns] = np.bitwise_count((b & sh) & pairs).sum(axis=1, dtype=np.uint32)
        return t1 - t0, time.perf_counter() - t1
    run(0, chunk)                                                     # warm-up: staging buffers, code objects, the host buffer's pages
    passes = []
    for _ in range(args.route_repeats):
        d = p = 0.0
        for s0 in range(0, L, chunk):
            a, b = run(s0, min(chunk, L - s0))
            d += a; p += b
        passes.append({"download_s": d, "popcount_s": p, "total_s": d + p})
    passes.sort(key=lambda r: r["total_s"])
    rec = {"step": "snp_major", "n_ind": n, "n_loci": L, "repeats": args.route_repeats, "chunk_snps": chunk, "bytes_downloaded": L * w * 8,
           "passes": passes, "total_median_s": passes[len(passes) // 2]["total_s"], "sha256": digest(het, hom)}
    ctx.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_ind", nargs="?", type=int, default=100_000)
    ap.add_argument("n_loci", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--route-repeats", type=int, default=1)
    ap.add_argument("--route-chunk", type=int, default=32768)
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    args = ap.parse_args()
    if args.step:
        {"counts": step_counts, "snp_major": step_snp_major}[args.step](args)
        return 0
    recs = {}
    for step in ("counts", "snp_major"):
        cmd = [sys.executable, os.path.abspath(__file__), str(args.n_ind), str(args.n_loci), "--repeats", str(args.repeats),
               "--route-repeats", str(args.route_repeats), "--route-chunk", str(args.route_chunk), "--step", step]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S[step])
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": step, "error": f"no result within {STEP_LIMIT_S[step]} s"}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"step": step, "error": f"exit status {r.returncode}"}), flush=True)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        recs[step] = json.loads(line)
    c, s = recs["counts"], recs["snp_major"]
    print(json.dumps({"summary": "snp_counts_rate", "n_ind": args.n_ind, "n_loci": args.n_loci, "counts_call_median_ms": 1e3 * c["call_median_s"],
                      "counts_fixed_cost_median_ms": 1e3 * c["fixed_cost_median_s"], "counts_fraction_of_8TBps": c["fraction_of_8TBps"],
                      "snp_major_route_s": s["total_median_s"], "route_over_counts": s["total_median_s"] / c["call_median_s"],
                      "counts_agree": c["sha256"] == s["sha256"]}), flush=True)
    return 0 if c["sha256"] == s["sha256"] else 1


if __name__ == "__main__":
    sys.exit(main())
