#!/usr/bin/env python3
"""Rate of gev_snp_trait_sums (per-SNP trait sums from the resident rows on the matrix cores, csrc/gev_traitsum.h: the integers of an
association scan) at BASELINE config 2's shape (100 000 individuals, 1 M SNPs), beside the route it replaces: gev_download_snp_major
of the same SNPs plus a matrix product on the host.  Synthetic founders, one generation, random quanta over the whole +-2^30.

    python tools/assoc_rate.py [n_ind] [n_loci] [--traits 4,16] [--repeats 5] [--host-snps 8192] [--run 2048]

Every GPU step runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.  One JSON
line per step, then one summary line per number of traits:
  scan        one chromosome-wide gev_snp_trait_sums call over all individuals, all four outputs, host to host: median of --repeats after
              a warm-up; the same call over one individual (the fixed cost: the SNP-major passes, the launches, the copies); the bytes the
              design cannot go below (the transpose reads the rows and writes them SNP-major, the preparation reads them once more:
              3 x n_loci x n_ind / 4 bytes) over the median as a fraction of 8 TB/s
  download    SNPs [0, --host-snps) through gev_download_snp_major in runs of --run SNPs and a float64 BLAS product of the unpacked
              genotypes with the quanta (exact: every partial sum stays below 2^53), both timed in full and scaled to the chromosome
The steps build the same population and the same quanta from the same seeds; the summary says whether the sums of the first --host-snps
SNPs are equal (SHA-256) and gives the ratio of the download route to the device call."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
STEP_LIMIT_S = {"scan": 600, "download": 600}


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


def quanta(n_traits, n):
    import numpy as np
    return np.random.RandomState(99).randint(-(1 << 30), (1 << 30) + 1, size=(n_traits, n), dtype=np.int64).astype(np.int32)


def digest(arrays):
    return hashlib.sha256(b"".join(a.astype("<i8").tobytes() for a in arrays)).hexdigest()


def median(times):
    return sorted(times)[len(times) // 2]


def step_scan(args):
    import ctypes as C
    import numpy as np
    from geneevolve_amd import capi
    n, L, T = args.n_ind, args.n_loci, args.n_traits
    ctx = population(n, L)
    q = quanta(T, n)
    f = ctx.L._f("snp_trait_sums")
    gsum = np.empty((T, L), dtype=np.int64); hetsum = np.empty((T, L), dtype=np.int64)
    het = np.empty(L, dtype=np.uint32); hom = np.empty(L, dtype=np.uint32)

    def call(ns, ni, trait):                                          # (into the same host pages every time)
        t0 = time.perf_counter()
        ctx.L.check(f(ctx.h, 0, 0, 0, ns, 0, ni, trait, T, gsum, hetsum, het, hom))
        return time.perf_counter() - t0
    one = np.ascontiguousarray(q[:, :1])
    call(min(L, 4096), n, q); call(L, n, q)                           # warm-up: the CSR lists, the buffers, the code objects, the host pages
    times = [call(L, n, q) for _ in range(args.repeats)]
    H = min(args.host_snps, L)
    sha = digest([gsum[:, :H], hetsum[:, :H], het[:H], hom[:H]])
    call(L, 1, one)
    fixed = [call(L, 1, one) for _ in range(args.repeats)]
    med = median(times)
    floor_bytes = 3 * L * n // 4
    rec = {"step": "scan", "n_ind": n, "n_loci": L, "n_traits": T, "repeats": args.repeats, "call_s": sorted(times), "call_median_s": med,
           "one_individual_call_s": sorted(fixed), "one_individual_median_s": median(fixed), "floor_bytes": floor_bytes,
           "fraction_of_8TBps": floor_bytes / med / HBM_BYTES_PER_S, "genotype_trait_products_per_s": L * n * T / med,
           "result_bytes": int(gsum.nbytes + hetsum.nbytes + het.nbytes + hom.nbytes), "host_snps": H, "sha256_host_snps": sha}
    ctx.close()
    print(json.dumps(rec), flush=True)


def step_download(args):
    import numpy as np
    from geneevolve_amd import capi
    n, L, T = args.n_ind, args.n_loci, args.n_traits
    ctx = population(n, L)
    q = quanta(T, n).astype(np.float64).T.copy()                      # [n][T]
    ctx.download_snp_major(0, 0, 0, 64)                               # warm-up: the CSR lists, the staging buffer
    H = min(args.host_snps, L)
    gsum = np.empty((T, H), dtype=np.int64); hetsum = np.empty((T, H), dtype=np.int64)
    het = np.empty(H, dtype=np.uint32); hom = np.empty(H, dtype=np.uint32)
    t_down = t_prod = 0.0
    nbytes = 0
    for s in range(0, H, args.run):
        ns = min(args.run, H - s)
        t0 = time.perf_counter()
        words = ctx.download_snp_major(0, 0, s, ns)
        t1 = time.perf_counter()
        h = capi.unpack_rows(np.ascontiguousarray(words[:, :capi.words_for(2 * n)]), 2 * n)
        g = (h[:, 0::2] + h[:, 1::2]).astype(np.float64)
        one = (g == 1.0).astype(np.float64)
        gsum[:, s:s + ns] = (g @ q).T.astype(np.int64); hetsum[:, s:s + ns] = (one @ q).T.astype(np.int64)
        het[s:s + ns] = one.sum(axis=1); hom[s:s + ns] = (g == 2.0).sum(axis=1)
        t2 = time.perf_counter()
        t_down += t1 - t0; t_prod += t2 - t1; nbytes += int(words.nbytes)
    rec = {"step": "download", "n_ind": n, "n_loci": L, "n_traits": T, "host_snps": H, "run": args.run, "download_s": t_down, "bytes_downloaded": nbytes,
           "products_s": t_prod, "download_s_scaled": t_down * L / H, "products_s_scaled": t_prod * L / H, "total_s_scaled": (t_down + t_prod) * L / H,
           "sha256_host_snps": digest([gsum, hetsum, het, hom])}
    ctx.close()
    print(json.dumps(rec), flush=True)


STEPS = {"scan": step_scan, "download": step_download}


def run_step(args, step, extra):
    cmd = [sys.executable, os.path.abspath(__file__), str(args.n_ind), str(args.n_loci), "--repeats", str(args.repeats), "--host-snps", str(args.host_snps),
           "--run", str(args.run), "--step", step] + extra
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S[step])
    except subprocess.TimeoutExpired:
        print(json.dumps({"step": step, "args": extra, "error": f"no result within {STEP_LIMIT_S[step]} s"}), flush=True)
        return None
    if r.returncode != 0:
        print(json.dumps({"step": step, "args": extra, "error": f"exit status {r.returncode}"}), flush=True)
        return None
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_ind", nargs="?", type=int, default=100_000)
    ap.add_argument("n_loci", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--traits", default="4,16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-snps", type=int, default=8192)
    ap.add_argument("--run", type=int, default=2048)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--n-traits", type=int)
    args = ap.parse_args()
    if args.step:
        STEPS[args.step](args)
        return 0
    ok = True
    for T in (int(v) for v in args.traits.split(",") if v):
        d = run_step(args, "scan", ["--n-traits", str(T)])
        h = d and run_step(args, "download", ["--n-traits", str(T)])
        if not h:
            return 1
        agree = d["sha256_host_snps"] == h["sha256_host_snps"]
        ok = ok and agree
        print(json.dumps({"summary": "assoc_rate", "n_ind": args.n_ind, "n_loci": args.n_loci, "n_traits": T, "device_call_median_s": d["call_median_s"],
                          "one_individual_median_s": d["one_individual_median_s"], "fraction_of_8TBps": d["fraction_of_8TBps"],
                          "download_s_scaled": h["download_s_scaled"], "host_products_s_scaled": h["products_s_scaled"], "download_route_s": h["total_s_scaled"],
                          "route_over_device": h["total_s_scaled"] / d["call_median_s"], "sums_agree": agree}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
