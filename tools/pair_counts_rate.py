#!/usr/bin/env python3
"""Rate of gev_pair_genotype_counts (pairwise genotype counts from the resident rows on the matrix cores, csrc/gev_paircount.h) at
BASELINE config 2's row shape (1 M SNPs), beside the only other route to the same numbers: gev_download_haps of the block's rows plus
numpy int32 products on the host.  Synthetic founders, one generation.

    python tools/pair_counts_rate.py [n_ind] [n_loci] [--blocks 1024,4096,8192] [--repeats 5] [--host-loci 2048]

Every GPU step runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.  One JSON
line per step, then one summary line per block size:
  device     one call for the block [0, B) x [0, B) over the whole chromosome, host to host (the call returns with the three matrices in
             host memory): median of --repeats after a warm-up; pair-loci per second, and that as a fraction of the int8 matrix rate
             for two products (2 x the dense bf16 peak of 2.5 PFLOP/s = 2.5e15 multiply-adds per second, so 1.25e15 pair-loci/s)
  download   the rows of the same B individuals through gev_download_haps (timed in full), then the three numpy int32 products
             (x @ x.T, y @ z.T + z @ y.T, g @ g.T).  numpy has no BLAS for integers: the products are timed over the first --host-loci
             SNPs at blocks of 1024 (fewer at larger blocks: the work is kept about the same) and scaled to the chromosome (`products_s_scaled`; `products_loci_timed` says over how many they ran)
The two steps build the same population from the same seeds; the summary says whether their counts over the first --host-loci SNPs
agree (SHA-256) and whether the device route is the faster one."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
I8_PAIR_LOCI_PER_S = 1.25e15
STEP_LIMIT_S = {"device": 420, "download": 600}


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


def host_loci(args):
    """the SNPs the host products are timed over: --host-loci at blocks of 1024, fewer for larger blocks (the work stays about the same)"""
    return min(args.n_loci, max(64, args.host_loci * 1024 * 1024 // (args.block * args.block) // 64 * 64))


def digest(mats):
    return hashlib.sha256(b"".join(m.astype("<u4").tobytes() for m in mats)).hexdigest()


def step_device(args):
    import ctypes as C
    import numpy as np
    from geneevolve_amd import capi
    n, L, B = args.n_ind, args.n_loci, args.block
    ctx = population(n, L)
    mats = [np.empty((B, B), dtype=np.uint32) for _ in range(3)]
    f = ctx.L._f("pair_genotype_counts")

    def call(ns, b):
        t0 = time.perf_counter()
        ctx.L.check(f(ctx.h, 0, 0, 0, ns, 0, b, 0, b, *mats))
        return time.perf_counter() - t0
    call(L, min(B, 256)); call(L, B)                                  # warm-up: the CSR lists, the buffers, the code objects, the host pages
    times = sorted(call(L, B) for _ in range(args.repeats))
    med = times[len(times) // 2]
    small = [np.empty((B, B), dtype=np.uint32) for _ in range(3)]
    hl = host_loci(args)
    ctx.L.check(f(ctx.h, 0, 0, 0, hl, 0, B, 0, B, *small))
    rec = {"step": "device", "n_ind": n, "n_loci": L, "block": B, "repeats": args.repeats, "call_s": times, "call_median_s": med,
           "pair_loci": B * B * L, "pair_loci_per_s": B * B * L / med, "fraction_of_i8_rate": B * B * L / med / I8_PAIR_LOCI_PER_S,
           "result_bytes": 3 * B * B * 4, "dot_trace": int(np.trace(mats[2]).astype(np.int64)), "sha256_host_loci": digest(small)}
    ctx.close()
    print(json.dumps(rec), flush=True)


def step_download(args):
    import numpy as np
    from geneevolve_amd import capi
    n, L, B = args.n_ind, args.n_loci, args.block
    ctx = population(n, L)
    ctx.download_haps(0, 0, 0, 2)                                      # warm-up: the CSR lists, the staging buffer
    t0 = time.perf_counter()
    words = ctx.download_haps(0, 0, 0, 2 * B)
    t_down = time.perf_counter() - t0
    hl = host_loci(args)
    t0 = time.perf_counter()
    bits = capi.unpack_rows(np.ascontiguousarray(words[:, :capi.words_for(hl)]), hl).astype(np.int32)
    a, b = bits[0::2], bits[1::2]
    x, y, zz, g = a ^ b, a & b, 1 - (a | b), a + b
    mats = [x @ x.T, y @ zz.T + zz @ y.T, g @ g.T]
    t_prod = time.perf_counter() - t0
    scaled = t_prod * L / hl
    rec = {"step": "download", "n_ind": n, "n_loci": L, "block": B, "download_s": t_down, "bytes_downloaded": int(words.nbytes),
           "products_loci_timed": hl, "products_s_timed": t_prod, "products_s_scaled": scaled, "total_s": t_down + scaled,
           "sha256_host_loci": digest(mats)}
    ctx.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_ind", nargs="?", type=int, default=100_000)
    ap.add_argument("n_loci", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--blocks", default="1024,4096,8192")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-loci", type=int, default=2048)
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    ap.add_argument("--block", type=int)
    args = ap.parse_args()
    if args.step:
        {"device": step_device, "download": step_download}[args.step](args)
        return 0
    ok = True
    for B in (int(v) for v in args.blocks.split(",")):
        if B > args.n_ind:
            print(json.dumps({"block": B, "error": f"more than the {args.n_ind} individuals"}), flush=True)
            return 1
        recs = {}
        for step in ("device", "download"):
            cmd = [sys.executable, os.path.abspath(__file__), str(args.n_ind), str(args.n_loci), "--repeats", str(args.repeats),
                   "--host-loci", str(args.host_loci), "--step", step, "--block", str(B)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S[step])
            except subprocess.TimeoutExpired:
                print(json.dumps({"step": step, "block": B, "error": f"no result within {STEP_LIMIT_S[step]} s"}), flush=True)
                return 1
            if r.returncode != 0:
                print(json.dumps({"step": step, "block": B, "error": f"exit status {r.returncode}"}), flush=True)
                return 1
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            recs[step] = json.loads(line)
        d, h = recs["device"], recs["download"]
        agree = d["sha256_host_loci"] == h["sha256_host_loci"]
        ok = ok and agree and d["call_median_s"] < h["total_s"]
        print(json.dumps({"summary": "pair_counts_rate", "n_ind": args.n_ind, "n_loci": args.n_loci, "block": B, "device_call_median_s": d["call_median_s"],
                          "device_pair_loci_per_s": d["pair_loci_per_s"], "device_fraction_of_i8_rate": d["fraction_of_i8_rate"],
                          "download_s": h["download_s"], "host_products_s_scaled": h["products_s_scaled"], "download_route_s": h["total_s"],
                          "route_over_device": h["total_s"] / d["call_median_s"], "device_faster": d["call_median_s"] < h["total_s"],
                          "counts_agree": agree}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
