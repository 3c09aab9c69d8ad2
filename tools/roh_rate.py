#!/usr/bin/env python3
"""Rate of gev_roh_summary and gev_roh_segments (runs of homozygosity scanned on the device from the staged rows, csrc/gev_roh.h) on
a whole population, beside the route they replace measured in the same process: gev_download_haps of the same individuals plus
gev_dbg_roh_host on one CPU core.

    python tools/roh_rate.py [n_ind] [--snps 100000] [--gens 10] [--min-snps 100] [--repeats 5] [--out profiles/NAME.jsonl]

One JSON line (also appended to --out), medians over the repeats after a warm-up of every call:
  summary_s     gev_roh_summary with all five outputs (the rows staged and scanned once, the cover's prefix sum, 24 bytes an individual
                and 4 bytes a SNP back)
  count_only_s  gev_roh_segments with out NULL (staged and scanned once, one 8-byte total back per pass)
  full_s        gev_roh_segments with a buffer of n_total records (count, scan, fill with a second walk, 32 bytes a record back; a
                request of several passes stages and counts every pass twice)
  download_s    gev_download_haps of all rows: what the host route moves before it can begin
  host_walk_s   gev_dbg_roh_host on those rows with all outputs and the list, one core (its count and its fill, as the device call's)
  equal_host    the device gave the same six results as the host walk
`passes` is the number of staging passes of a call; `row_bytes` the bytes of the rows one scan reads."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def population(n, n_snps, gens):
    from geneevolve_amd.capi import GevLibrary
    from geneevolve_amd.host import Simulation, SyntheticConfig
    cfg = SyntheticConfig(n, n_snps, n_cv=1000, seed=12345)
    ctx = GevLibrary().create(1, 1, 1, 0)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 31); ctx.synth_cv_founders(0, 0, 0, 2 * n, 77)
    sim = Simulation(ctx, 1, 1, True)
    sim.ras_initial_human_gen0(0, n)
    for _ in range(gens):
        sim.next_generation_rm(0, n)
    ctx.sync()
    return ctx, cfg


def median(x):
    return sorted(x)[len(x) // 2]


def timed(call):
    t0 = time.perf_counter()
    r = call()
    return time.perf_counter() - t0, r


def main():
    import numpy as np
    from geneevolve_amd.capi import ROH_SEGMENT_DTYPE, _roh_outs, _roh_params
    ap = argparse.ArgumentParser()
    ap.add_argument("n_ind", nargs="?", type=int, default=20_000)
    ap.add_argument("--snps", type=int, default=100_000)
    ap.add_argument("--gens", type=int, default=10)
    ap.add_argument("--min-snps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    n, L = args.n_ind, args.snps
    ctx, cfg = population(n, L, args.gens)
    q = _roh_params(args.min_snps)
    outs = _roh_outs(n, L)
    for o in outs:
        o[:] = 0                                                   # (the host pages exist)
    f, g = ctx.L._f("roh_summary"), ctx.L._f("roh_segments")
    total = C.c_uint64()

    def summary():
        ctx.L.check(f(ctx.h, 0, 0, 0, L, 0, n, C.byref(q), *outs))

    def segments(out, capacity):
        ctx.L.check(g(ctx.h, 0, 0, 0, L, 0, n, C.byref(q), out, capacity, C.byref(total)))
    summary(); segments(None, 0)                                   # warm-up: the CSR lists, the buffers, the code object
    n_total = int(total.value)
    rec = np.zeros(max(n_total, 1), dtype=ROH_SEGMENT_DTYPE)
    segments(rec, n_total)
    t_sum, t_cnt, t_full = [], [], []
    for _ in range(args.repeats):
        t_sum.append(timed(summary)[0]); t_cnt.append(timed(lambda: segments(None, 0))[0]); t_full.append(timed(lambda: segments(rec, n_total))[0])
    ctx.download_haps(0, 0, 0, 2)
    t_down = []
    for _ in range(args.repeats):
        t, words = timed(lambda: ctx.download_haps(0, 0))
        t_down.append(t)
    stride = -(-L // 1024) * 128                                   # bytes of a staged row: a multiple of 128
    per_pass = max((256 << 20) // (2 * stride), 1)                 # individuals of a staging pass
    lib = ctx.L
    ctx.close()
    lib.dbg_roh_host(words[:64], L, cfg.snp_pos, min_snps=args.min_snps)
    t_host, host = timed(lambda: lib.dbg_roh_host(words, L, cfg.snp_pos, min_snps=args.min_snps))
    equal = all(a.tobytes() == b.tobytes() for a, b in zip((*outs, rec[:n_total]), host))
    line = json.dumps({"n_ind": n, "n_snps": L, "generations": args.gens, "min_snps": args.min_snps, "repeats": args.repeats,
                       "row_bytes": 2 * n * stride, "passes": -(-n // per_pass), "n_total": n_total, "record_bytes": n_total * ROH_SEGMENT_DTYPE.itemsize,
                       "individuals_with_a_run": int((outs[0] > 0).sum()), "roh_snps": int(outs[2].sum(dtype=np.uint64)),
                       "summary_call_s": t_sum, "summary_s": median(t_sum), "count_only_call_s": t_cnt, "count_only_s": median(t_cnt),
                       "full_call_s": t_full, "full_s": median(t_full), "download_call_s": t_down, "download_s": median(t_down),
                       "host_walk_s": t_host, "equal_host": bool(equal), "device_before_download": bool(max(median(t_sum), median(t_full)) < median(t_down)),
                       "sha256": hashlib.sha256(rec[:n_total].tobytes()).hexdigest()})
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
