#!/usr/bin/env python3
"""Rate of gev_ibd_sharing (identity by descent per pair of haplotype rows walked from the ancestry interval lists, csrc/gev_ibd.h) on a
block of rows of a large population without genotype planes, at several ages of the run: the lists lengthen by about one part per
generation at the default map (one crossover per gamete and generation).

    python tools/ibd_rate.py [n_ind] [--block 4096] [--gens 10,100,300] [--repeats 5] [--host-block 256] [--out profiles/ibd_rate_NAME.jsonl]

Every age runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.  One JSON line
per configuration (also appended to --out):
  device   the block [0, B) x [0, B) of haplotype rows after a warm-up.  `call_s`: the whole call host to host with the three matrices
           wanted (20 bytes a pair are copied out); `seg_only_call_s`: the same with n_seg alone (4 bytes a pair): the walk is the same,
           the copy a fifth.  Rates are given over the median of the second: pairs per second, and walk steps per second, a pair's
           steps being the lengths of its two lists summed.
  host     for context only: gev_dbg_ibd_host (the same walk compiled for the host) on one CPU core over rows [0, H) x [0, H) of the
           lists downloaded from the same population; `equal_device` says that the device gave the same integers there."""
import argparse
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


def digest(mats):
    return hashlib.sha256(b"".join(m.tobytes() for m in mats)).hexdigest()


def step(args):
    import numpy as np
    n, B, H, gens = args.n_ind, args.block, args.host_block, args.step_gens
    ctx = population(n, gens)
    n_parts = ctx.ancestry_bp(0, 0, 0, B)[1].astype(np.int64)
    steps = int(B * n_parts.sum() * 2)                              # sum over the pairs of both list lengths
    outs = [np.empty((B, B), dtype=dt) for dt in (np.uint64, np.uint32, np.uint64)]
    f = ctx.L._f("ibd_sharing")

    def call(all_three):
        t0 = time.perf_counter()
        ctx.L.check(f(ctx.h, 0, 0, 0, B, 0, 0, B, 0, *(outs if all_three else (None, outs[1], None))))
        return time.perf_counter() - t0
    call(True); call(False)                                        # warm-up: the CSR lists, the buffers, the code object, the host pages
    full, seg = [], []
    for _ in range(args.repeats):
        full.append(call(True)); seg.append(call(False))
    med = sorted(seg)[len(seg) // 2]
    print(json.dumps({"step": "device", "n_ind": n, "generations": gens, "block": B, "repeats": args.repeats, "parts_per_row_mean": float(n_parts.mean()),
                      "parts_per_row_max": int(n_parts.max()), "pairs": B * B, "walk_steps": steps, "call_s": full, "call_median_s": sorted(full)[len(full) // 2],
                      "seg_only_call_s": seg, "seg_only_median_s": med, "pairs_per_s": B * B / med, "walk_steps_per_s": steps / med,
                      "shared_bp_trace": int(np.trace(outs[0]).astype(np.uint64)), "sha256": digest(outs)}), flush=True)
    parts, off = ctx.download_intervals(0, 0)
    lib = ctx.L
    ctx.close()
    off_h = off[:H + 1]
    t0 = time.perf_counter()
    host = lib.dbg_ibd_host(parts, off_h)
    t = time.perf_counter() - t0
    h_steps = int(H * np.diff(off_h.astype(np.int64)).sum() * 2)
    print(json.dumps({"step": "host", "n_ind": n, "generations": gens, "block": H, "call_s": t, "pairs_per_s": H * H / t, "walk_steps_per_s": h_steps / t,
                      "equal_device": bool(all(np.array_equal(h, o[:H, :H]) for h, o in zip(host, outs)))}), flush=True)


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
