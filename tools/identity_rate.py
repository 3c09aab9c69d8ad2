#!/usr/bin/env python3
"""Time of gev_identity_states (csrc/gev_identity.h: Jacquard's nine identity states per pair of individuals, walked on the device from
the ancestry interval lists) on a block of individuals of a large population without genotype planes, at several ages of the run,
against the route the call replaces: gev_download_intervals of the population and the four-list merge of the same header compiled
stand-alone on one host core (tools/identity_merge_host.cpp; numpy has no vectorised form of it).

    python tools/identity_rate.py [n_ind] [--block 2048] [--gens 10,100,300] [--runs 3] [--host-lib PATH] [--out profiles/identity_rate.jsonl]

--host-lib: the library the replaced route and the haplotype-pair call run on (a build of the commit before the call existed); without
it, this build's.  Every age runs in a process of its own under its own time limit; a step that fails or runs out of time ends the
run.  In a step both populations are bred from the same seeds and the routes run alternately (host route, device, haplotype pairs,
...) after one warm-up each, every call timed host to host.  One JSON line per run and a summary line per age (also appended to --out):
  device      gev_identity_states over individuals [0, B) x [0, B): 9 planes, 72 bytes a pair, in the caller's memory when it returns
  host_route  gev_download_intervals of the population, then the merge over the same block; `equal` says both gave the same bytes,
              `bar` that every device run was shorter than every host-route run
  hap_pairs   recorded, not barred: gev_ibd_sharing with shared_bp alone over the same 2 B x 2 B haplotype rows, the only per-pair number
              there was before (8 bytes a pair of rows = 32 a pair of individuals)
`walk_steps` = over the pairs of individuals the summed lengths of their four lists (every step of a walk moves a list on)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 540
MERGE_SRC = os.path.join(ROOT, "tools", "identity_merge_host.cpp")
MERGE_LIB = os.path.join(ROOT, "tools", "libidentity_merge_host.so")


def population(lib, n, gens):
    from geneevolve_amd.host import Simulation, SyntheticConfig
    cfg = SyntheticConfig(n, 4096, n_cv=1000, seed=12345)
    ctx = lib.create(1, 1, 1, 0)
    ctx.set_dense_state(False)
    cfg.apply_static(ctx)
    ctx.synth_cv_founders(0, 0, 0, 2 * n, 77)
    sim = Simulation(ctx, 1, 1, True)
    sim.ras_initial_human_gen0(0, n)
    for _ in range(gens):
        sim.next_generation_rm(0, n)
    ctx.sync()
    return ctx


def merge_library():
    if not os.path.exists(MERGE_LIB) or os.path.getmtime(MERGE_LIB) < os.path.getmtime(MERGE_SRC):
        subprocess.run(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", MERGE_SRC, "-o", MERGE_LIB], check=True)
    f = ctypes.CDLL(MERGE_LIB).identity_merge_host
    f.restype = None
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    return f


def step(args):
    import numpy as np
    from geneevolve_amd.capi import GevLibrary
    n, B, gens = args.n_ind, args.block, args.step_gens
    lib = GevLibrary()
    ctx = population(lib, n, gens)
    hctx = population(GevLibrary(args.host_lib), n, gens) if args.host_lib else ctx
    merge = merge_library()
    n_parts = ctx.ancestry_bp(0, 0, 0, 2 * B)[1].astype(np.int64)
    steps = int(2 * B * n_parts.sum())                                 # every individual's two lists meet B partners, on either side
    dev_bp = np.empty((9, B, B), dtype=np.uint64); host_bp = np.empty((9, B, B), dtype=np.uint64); sh = np.empty((2 * B, 2 * B), dtype=np.uint64)
    f_dev, f_sh = ctx.L._f("identity_states"), hctx.L._f("ibd_sharing")

    def device():
        t0 = time.perf_counter()
        ctx.L.check(f_dev(ctx.h, 0, 0, 0, B, 0, 0, B, dev_bp))
        return time.perf_counter() - t0

    def host_route(block):
        t0 = time.perf_counter()
        parts, off = hctx.download_intervals(0, 0)
        t1 = time.perf_counter()
        merge(parts.ctypes.data, off.ctypes.data, 0, block, 0, block, host_bp.ctypes.data)
        return time.perf_counter() - t0, t1 - t0

    def hap_pairs():
        t0 = time.perf_counter()
        hctx.L.check(f_sh(hctx.h, 0, 0, 0, 2 * B, 0, 0, 2 * B, 0, sh, None, None))
        return time.perf_counter() - t0
    device(); host_route(min(B, 64)); hap_pairs()                      # warm-up: the CSR lists, the buffers, the code objects, the host pages
    lines, dev_s, host_s, dl_s, hap_s, equal = [], [], [], [], [], True

    def emit(rec):
        lines.append(json.dumps({"generations": gens, **rec}))
        print(lines[-1], flush=True)
    for k in range(args.runs):
        t, dl = host_route(B)
        host_s.append(t); dl_s.append(dl)
        emit({"step": "host_route", "run": k, "call_s": t, "download_s": dl, "library": "the --host-lib build" if args.host_lib else "this build"})
        dev_s.append(device())
        same = dev_bp.tobytes() == host_bp.tobytes()
        equal = equal and same
        emit({"step": "device", "run": k, "call_s": dev_s[-1], "equal_host_route": same})
        hap_s.append(hap_pairs())
        emit({"step": "hap_pairs", "run": k, "call_s": hap_s[-1]})
    med = lambda v: sorted(v)[len(v) // 2]
    total = dev_bp.sum(axis=0, dtype=np.uint64)
    emit({"step": "summary", "n_ind": n, "block": B, "pairs": B * B, "parts_per_row_mean": float(n_parts.mean()), "parts_per_row_max": int(n_parts.max()),
          "walk_steps": steps, "bytes_out": 72 * B * B, "device_s": dev_s, "host_route_s": host_s, "host_download_s": dl_s, "hap_pairs_s": hap_s,
          "device_max_s": max(dev_s), "host_route_min_s": min(host_s), "ratio_min_host_over_max_device": min(host_s) / max(dev_s),
          "device_over_hap_pairs_median": med(dev_s) / med(hap_s), "walk_steps_per_s": steps / med(dev_s), "host_walk_steps_per_s": steps / (med(host_s) - med(dl_s)),
          "equal": equal, "bar": max(dev_s) < min(host_s),
          "state_share": [float(x) for x in dev_bp.reshape(9, -1).sum(axis=1, dtype=np.uint64) / float(total.sum(dtype=np.uint64))],
          "kinship_identity": bool(np.array_equal(np.uint64(4) * dev_bp[0] + np.uint64(2) * (dev_bp[2] + dev_bp[4] + dev_bp[6]) + dev_bp[7],
                                                  sh[0::2, 0::2] + sh[0::2, 1::2] + sh[1::2, 0::2] + sh[1::2, 1::2]))})
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_ind", nargs="?", type=int, default=100_000)
    ap.add_argument("--block", type=int, default=2048)
    ap.add_argument("--gens", default="10,100,300")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-lib")
    ap.add_argument("--out")
    ap.add_argument("--step-gens", type=int)
    args = ap.parse_args()
    if args.step_gens is not None:
        return step(args)
    if args.block > args.n_ind:
        print(json.dumps({"error": "the block does not fit the population"}), flush=True)
        return 1
    for gens in (int(v) for v in args.gens.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), str(args.n_ind), "--block", str(args.block), "--runs", str(args.runs), "--step-gens", str(gens)]
        cmd += (["--host-lib", args.host_lib] if args.host_lib else []) + (["--out", args.out] if args.out else [])
        try:
            r = subprocess.run(cmd, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps({"generations": gens, "error": f"no result within {STEP_LIMIT_S} s"}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"generations": gens, "error": f"exit status {r.returncode}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
