#!/usr/bin/env python3
"""Rate of gev_ibd_segments (the IBD segments of pairs of haplotype rows listed on the device, csrc/gev_ibd.h) on a block of rows of a
large population without genotype planes, in GEV_IBD_UPPER mode, at several ages of the run, beside two yardsticks measured in the
same process: gev_ibd_sharing on the same block, and the route the call replaces.

    python tools/ibd_segments_rate.py [n_ind] [--block 4096] [--gens 10,100,300] [--repeats 5] [--host-block 256] [--out profiles/NAME.jsonl]

Every age runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.  One JSON line
per configuration (also appended to --out):
  device   the block [0, B) x [0, B), pairs with row_a < row_b, after a warm-up, medians over the repeats.  `count_only_s`: the call with
           out NULL (one walk, one 8-byte total back per strip); `full_s`: the call with a buffer of n_total records (count, scan, fill
           with a second walk, copy-out of 24 bytes a record); `records_per_s` over the median of the second.  `sharing_s`:
           gev_ibd_sharing on the same block with all three matrices (one walk of all B x B pairs, 20 bytes a pair out).
  host     the route it replaces: gev_download_intervals (timed as it is, the whole population's lists) and gev_dbg_ibd_segments_host on
           one CPU core over rows [0, H) x [0, H) in upper mode; `scaled_block_s` is that walk's time times (B / H)^2, an estimate
           and labelled so; `equal_device` says that the device gave the same records for those rows."""
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
STEP_LIMIT_S = 540


def population(n, gens):
    from geneevolve_amd.capi import GevLibrary
    from geneevolve_amd.host import Simulation, SyntheticConfig
    cfg = SyntheticConfig(n, 4096, n_cv=1000, seed=12345)
    ctx = GevLibrary().create(1, 1, 1, 0)
    ctx.set_dense_state(False)
    cfg.apply_static(ctx)
    ctx.synth_cv_founders(0, 0, 0, 2 * n, 77)
    sim = Simulation(ctx, 1, 1, True)
    sim.ras_initial_human_gen0(0, n)
    for _ in range(gens):
        sim.next_generation_rm(0, n)
    ctx.sync()
    return ctx


def median(x):
    return sorted(x)[len(x) // 2]


def step(args):
    import numpy as np
    from geneevolve_amd.capi import IBD_UPPER, SEGMENT_DTYPE
    n, B, H, gens = args.n_ind, args.block, args.host_block, args.step_gens
    ctx = population(n, gens)
    n_parts = ctx.ancestry_bp(0, 0, 0, B)[1].astype(np.int64)
    f = ctx.L._f("ibd_segments")
    total = C.c_uint64()

    def call(out, capacity):
        t0 = time.perf_counter()
        ctx.L.check(f(ctx.h, 0, 0, 0, B, 0, 0, B, 0, IBD_UPPER, out, capacity, C.byref(total)))
        return time.perf_counter() - t0
    call(None, 0)                                                  # warm-up: the CSR lists, the buffers, the code object
    n_total = int(total.value)
    out = np.zeros(max(n_total, 1), dtype=SEGMENT_DTYPE)           # (zeroed: the host pages exist)
    call(out, n_total)
    count_only, full = [], []
    for _ in range(args.repeats):
        count_only.append(call(None, 0)); full.append(call(out, n_total))
    mats = [np.empty((B, B), dtype=dt) for dt in (np.uint64, np.uint32, np.uint64)]
    g = ctx.L._f("ibd_sharing")

    def sharing():
        t0 = time.perf_counter()
        ctx.L.check(g(ctx.h, 0, 0, 0, B, 0, 0, B, 0, *mats))
        return time.perf_counter() - t0
    sharing()
    shared = [sharing() for _ in range(args.repeats)]
    consistent = bool(n_total == int(np.triu(mats[1], 1).sum(dtype=np.uint64)))
    print(json.dumps({"step": "device", "n_ind": n, "generations": gens, "block": B, "pairs": "upper", "repeats": args.repeats,
                      "parts_per_row_mean": float(n_parts.mean()), "parts_per_row_max": int(n_parts.max()), "n_pairs": B * (B - 1) // 2, "n_total": n_total,
                      "record_bytes": n_total * SEGMENT_DTYPE.itemsize, "count_only_call_s": count_only, "count_only_s": median(count_only),
                      "full_call_s": full, "full_s": median(full), "records_per_s": n_total / median(full),
                      "sharing_call_s": shared, "sharing_s": median(shared), "n_total_equals_sharing_n_seg": consistent,
                      "sha256": hashlib.sha256(out[:n_total].tobytes()).hexdigest()}), flush=True)
    t0 = time.perf_counter()
    parts, off = ctx.download_intervals(0, 0)
    t_down = time.perf_counter() - t0
    lib = ctx.L
    ctx.close()
    off_h = off[:H + 1]
    lib.dbg_ibd_segments_host(parts, off_h, upper=True)
    t0 = time.perf_counter()
    host = lib.dbg_ibd_segments_host(parts, off_h, upper=True)      # (the wrapper's two calls: a count and a fill, as the device call's)
    t = time.perf_counter() - t0
    dev = out[:n_total]
    dev = dev[(dev["row_a"] < H) & (dev["row_b"] < H)]
    print(json.dumps({"step": "host", "n_ind": n, "generations": gens, "block": H, "download_intervals_all_rows_s": t_down, "walk_s": t,
                      "records": int(len(host)), "scaled_block": B, "scaled_block_s": t * (B / H) ** 2, "scaled": True,
                      "equal_device": bool(host.tobytes() == dev.tobytes())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_ind", nargs="?", type=int, default=100_000)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--gens", default="10,100,300")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-block", type=int, default=256)
    ap.add_argument("--out")
    ap.add_argument("--step-gens", type=int)
    args = ap.parse_args()
    if args.step_gens is not None:
        step(args)
        return 0
    if args.block > 2 * args.n_ind or args.host_block > args.block:
        print(json.dumps({"error": "the blocks do not fit the population"}), flush=True)
        return 1
    for gens in (int(v) for v in args.gens.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), str(args.n_ind), "--block", str(args.block), "--repeats", str(args.repeats),
               "--host-block", str(args.host_block), "--step-gens", str(gens)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps({"generations": gens, "error": f"no result within {STEP_LIMIT_S} s"}), flush=True)
            return 1
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        for ln in lines:
            print(ln, flush=True)
        if args.out and lines:
            with open(args.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        if r.returncode != 0:
            print(json.dumps({"generations": gens, "error": f"exit status {r.returncode}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
