#!/usr/bin/env python3
"""Time of gev_founder_counts (csrc/gev_lineage.h: per position the site record and the rows by root population, over all rows) on a
large population without genotype planes, against the route the call replaces: gev_download_intervals of the whole population, a
numpy searchsorted per row and a bincount per position that give the same integers.

    python tools/lineage_rate.py [n_ind] [--gens 50] [--positions 1024] [--runs 3] [--host-lib PATH] [--out profiles/lineage_rate.jsonl]
    python tools/lineage_rate.py [n_ind] --device-only      (one warm-up and one call: the run to put under a kernel trace)

--host-lib: the library the host route runs on (a build of the commit before the call existed); without it, this build's.  Both routes
run in one process on populations bred from the same seeds, alternately (host, device, host, device, ...) after one warm-up each, every
call timed host to host: the device route returns when the results are in the caller's memory, the host route ends with its last
bincount.  One JSON line per run and a summary line (also appended to --out): `equal` says that both routes gave the same bytes, `bar`
that every device run was shorter than every host-route run.  The summary counts what the kernels read, for rates over a kernel trace's
times: `parts_read` = the parts of all rows once per batch of positions (each batch's cursors pass over every row's list once),
`label_bytes` = positions x founder tiles x rows x 4."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    return ctx, cfg


def host_route(ctx, pos, nfh):
    """(site, pop_counts) as gev_founder_counts gives them, from a download of every list"""
    import numpy as np
    from geneevolve_amd.capi import LINEAGE_SITE_DTYPE, NO_FOUNDER
    parts, off = ctx.download_intervals(0, 0)
    st, en, hap, rp = (np.ascontiguousarray(parts[k]) for k in ("st", "en", "hap_index", "root_population"))
    ends = np.cumsum(nfh).astype(np.uint64)
    base = np.r_[np.uint64(0), ends[:-1]].astype(np.uint64)
    F, n_rows = int(ends[-1]), len(off) - 1
    by_row = np.full((n_rows, len(pos)), NO_FOUNDER, dtype=np.uint32)
    o = off.astype(np.int64)
    for r in range(n_rows):
        a, b = o[r], o[r + 1]
        if a == b:
            continue
        q = np.minimum(np.searchsorted(en[a:b], pos, side="right"), b - a - 1) + a       # the first part with en > x, or the last one
        cov = (st[q] <= pos) & (pos < en[q])
        by_row[r, cov] = (base[rp[q]] + hap[q])[cov]
    fid = np.ascontiguousarray(by_row.T)
    site = np.zeros(len(pos), dtype=LINEAGE_SITE_DTYPE)
    pop_counts = np.zeros((len(pos), len(nfh)), dtype=np.uint32)
    edges = np.r_[base, ends[-1]].astype(np.int64)
    for p in range(len(pos)):
        ids = fid[p][fid[p] != NO_FOUNDER]
        c = np.bincount(ids, minlength=F)
        top = int(c.max()) if F else 0
        site[p] = (int((c.astype(np.uint64) ** 2).sum()), int(c.sum()), int((c != 0).sum()), top, int(c.argmax()) if top else NO_FOUNDER)
        pop_counts[p] = [c[edges[k]:edges[k + 1]].sum() for k in range(len(nfh))]
    return site, pop_counts, len(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_ind", nargs="?", type=int, default=100_000)
    ap.add_argument("--gens", type=int, default=50)
    ap.add_argument("--positions", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-lib")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    from geneevolve_amd.capi import GevLibrary
    lib = GevLibrary()
    n, lines = args.n_ind, []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    ctx, cfg = population(lib, n, args.gens)
    lo, hi = int(cfg.rmap_bp[0]), int(cfg.rmap_bp[-1])
    pos = np.linspace(lo, hi, args.positions, endpoint=False).astype(np.uint64)
    nfh = ctx.founder_haps()

    def device():
        t0 = time.perf_counter()
        _, site, pc = ctx.founder_counts(0, 0, pos, want=("site", "pop_counts"))
        return time.perf_counter() - t0, site, pc
    n_parts = int(ctx.ancestry_bp(0, 0)[1].astype(np.int64).sum())
    tile = lib.dbg_lineage_tile()
    n_tiles = max(-(-int(nfh.sum()) // tile), 1)
    batch = min(max((256 << 20) // (2 * n * 4), 1), len(pos))
    shape = {"n_ind": n, "rows": 2 * n, "generations": args.gens, "positions": len(pos), "founders": int(nfh.sum()), "tile": tile, "tiles": n_tiles,
             "parts": n_parts, "parts_per_row_mean": n_parts / (2 * n), "batches": -(-len(pos) // batch),
             "parts_read": n_parts * -(-len(pos) // batch), "label_bytes": len(pos) * n_tiles * 2 * n * 4}
    device()                                                             # warm-up: the CSR lists, the buffers, the code objects, the host pages
    if args.device_only:
        t, site, _ = device()
        emit({"step": "device_only", **shape, "call_s": t, "n_lineages_mean": float(site["n_lineages"].mean())})
        return 0
    if args.host_lib:
        hctx, _ = population(GevLibrary(args.host_lib), n, args.gens)
    else:
        hctx = ctx
    host_route(hctx, pos[:8], nfh)                                       # warm-up
    dev_s, host_s, equal = [], [], True
    for k in range(args.runs):
        t0 = time.perf_counter()
        h_site, h_pc, _ = host_route(hctx, pos, nfh)
        host_s.append(time.perf_counter() - t0)
        emit({"step": "host_route", "run": k, "call_s": host_s[-1], "library": "the --host-lib build" if args.host_lib else "this build"})
        t, site, pc = device()
        dev_s.append(t)
        same = site.tobytes() == h_site.tobytes() and pc.tobytes() == h_pc.tobytes()
        equal = equal and same
        emit({"step": "device", "run": k, "call_s": t, "equal_host_route": same})
    emit({"step": "summary", **shape, "device_s": dev_s, "host_route_s": host_s, "device_max_s": max(dev_s), "host_route_min_s": min(host_s),
          "ratio_min_host_over_max_device": min(host_s) / max(dev_s), "equal": equal, "bar": max(dev_s) < min(host_s),
          "n_lineages_mean": float(site["n_lineages"].mean()), "n_covered_min": int(site["n_covered"].min())})
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
