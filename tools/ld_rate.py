#!/usr/bin/env python3
"""Rate of gev_ld_counts and gev_ld_scores (SNP-pair counts and LD scores from the resident rows on the matrix cores, csrc/gev_ldcount.h)
at BASELINE config 2's shape (100 000 individuals = 200 000 haplotypes, 1 M SNPs), beside the route they replace:
gev_download_snp_major of the same SNPs plus matrix products on the host.  Synthetic founders, one generation.

    python tools/ld_rate.py [n_ind] [n_loci] [--blocks 1024,4096,8192] [--score-snps 100000] [--windows 500,1000] [--repeats 5] [--host-ind 2048]

Every GPU step runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.  One JSON
line per step, then one summary line per block size and per window:
  counts      one gev_ld_counts call for SNPs [0, B) x [B, 2B) over all individuals, both matrices, host to host: median of --repeats
              after a warm-up; pair-haplotypes per second (B * B * 2 n_ind / s) and that as a fraction of the int8 matrix rate for two
              products (1.25e15 pairs/s, the figure tools/pair_counts_rate.py uses); and where the time goes: the same call asked for
              the per-SNP vectors alone (the preparation of both sides) and for one matrix at a time
  scores      one gev_ld_scores call over --score-snps SNPs with w SNPs to either side (haplotype r^2): the band's pair-haplotypes per
              second against the rate for one product (2.5e15)
  download    the same SNPs through gev_download_snp_major alone (timed in full), then what the host has to do with them: the rows
              unpacked to float32 and the BLAS products (exact below 2^24), timed over the haplotypes of the first --host-ind
              individuals and scaled to all (`products_s_scaled`); for the scores a slice of 512 SNPs' windows, scaled to the band
The steps build the same population from the same seeds; the summary says whether the counts over the first --host-ind individuals
agree (SHA-256) and whether the device call beats the arrival of the rows alone."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
I8_PAIRS_PER_S = {2: 1.25e15, 1: 2.5e15}         # pairs of (SNP pair, summation index) per second at the int8 matrix rate, by products formed
STEP_LIMIT_S = {"counts": 300, "scores": 300, "download": 420, "download_scores": 420}


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


def digest(arrays):
    return hashlib.sha256(b"".join(a.astype("<u8").tobytes() for a in arrays)).hexdigest()


def median(times):
    return sorted(times)[len(times) // 2]


def unpack(words, n_hap):
    """SNP-major words -> float32 [n_snps][n_hap] of 0/1"""
    import numpy as np
    from geneevolve_amd import capi
    return capi.unpack_rows(np.ascontiguousarray(words[:, :capi.words_for(n_hap)]), n_hap).astype(np.float32)


def step_counts(args):
    n, L, B = args.n_ind, args.n_loci, args.block
    ctx = population(n, L)

    import ctypes as C
    import numpy as np
    from geneevolve_amd import capi
    f, mat, vec = ctx.L._f("ld_counts"), np.empty((B, B), dtype=np.uint32), np.empty(B, dtype=np.uint32)
    mats = [mat, np.empty((B, B), dtype=np.uint32)]

    def call(b, ni):                                                  # (into the same host pages every time)
        t0 = time.perf_counter()
        ctx.L.check(f(ctx.h, 0, 0, 0, b, 0, B, b, 0, ni, mats[0], mats[1], *[None] * 6))
        return time.perf_counter() - t0
    call(min(B, 256), n); call(B, n)                                  # warm-up: the CSR lists, the buffers, the code objects, the host pages
    times = [call(B, n) for _ in range(args.repeats)]
    med = median(times)
    call(B, args.host_ind)
    small = [m.copy() for m in mats]
    # where the call's time goes: the preparation of the two sides alone (only the per-SNP vectors asked for), one product with its copy-out

    def part(n11, gg):
        def once():
            t0 = time.perf_counter()
            ctx.L.check(f(ctx.h, 0, 0, 0, B, 0, B, B, 0, n, mat if n11 else None, mat if gg else None, vec, None, None, vec, None, None))
            return time.perf_counter() - t0
        once()
        return median([once() for _ in range(args.repeats)])
    parts = {"prepare_only_s": part(False, False), "n11_only_s": part(True, False), "gg_only_s": part(False, True)}
    pairs = B * B * 2 * n
    rec = {"step": "counts", "n_ind": n, "n_loci": L, "block": B, "repeats": args.repeats, "call_s": sorted(times), "call_median_s": med,
           "pair_haplotypes": pairs, "pair_haplotypes_per_s": pairs / med, "fraction_of_i8_rate": pairs / med / I8_PAIRS_PER_S[2],
           "result_bytes": 2 * B * B * 4, "sha256_host_ind": digest(small[:2]), **parts}
    ctx.close()
    print(json.dumps(rec), flush=True)


def step_scores(args):
    import numpy as np
    from geneevolve_amd import ld
    n, L, S, w = args.n_ind, args.n_loci, args.score_snps, args.window
    ctx = population(n, L)
    lo, hi = ld.windows_by_count(L, 0, S, w)

    def call(s, ni):
        t0 = time.perf_counter()
        out = ctx.ld_scores(0, 0, lo[:s], hi[:s], 0, s, 0, ni, False)
        return time.perf_counter() - t0, out
    call(min(S, 4096), n); call(S, n)
    times = [call(S, n)[0] for _ in range(args.repeats)]
    med = median(times)
    small = call(512, args.host_ind)[1]
    pairs = int((hi.astype(np.int64) - lo).sum()) * 2 * n
    rec = {"step": "scores", "n_ind": n, "n_loci": L, "score_snps": S, "window": w, "repeats": args.repeats, "call_s": sorted(times), "call_median_s": med,
           "band_pair_haplotypes": pairs, "pair_haplotypes_per_s": pairs / med, "fraction_of_i8_rate": pairs / med / I8_PAIRS_PER_S[1],
           "result_bytes": S * 12, "sha256_host_ind": digest(small)}
    ctx.close()
    print(json.dumps(rec), flush=True)


def step_download(args):
    import numpy as np
    n, L, B = args.n_ind, args.n_loci, args.block
    ctx = population(n, L)
    ctx.download_snp_major(0, 0, 0, 64)                               # warm-up: the CSR lists, the staging buffer
    t0 = time.perf_counter()
    words = ctx.download_snp_major(0, 0, 0, 2 * B)
    t_down = time.perf_counter() - t0
    nh = 2 * args.host_ind
    t0 = time.perf_counter()
    h = unpack(words, nh)
    g = h[:, 0::2] + h[:, 1::2]
    n11 = h[:B] @ h[B:].T; gg = g[:B] @ g[B:].T
    t_prod = time.perf_counter() - t0
    scaled = t_prod * (2 * n) / nh
    rec = {"step": "download", "n_ind": n, "n_loci": L, "block": B, "download_s": t_down, "bytes_downloaded": int(words.nbytes),
           "products_ind_timed": args.host_ind, "products_s_timed": t_prod, "products_s_scaled": scaled, "total_s": t_down + scaled,
           "sha256_host_ind": digest([n11, gg])}
    ctx.close()
    print(json.dumps(rec), flush=True)


def step_download_scores(args):
    import numpy as np
    from geneevolve_amd import ld
    from tests.ld_inputs import numpy_q40
    n, L, S, w = args.n_ind, args.n_loci, args.score_snps, args.window
    ctx = population(n, L)
    ctx.download_snp_major(0, 0, 0, 64)
    lo, hi = ld.windows_by_count(L, 0, S, w)
    t0 = time.perf_counter()
    words = ctx.download_snp_major(0, 0, 0, int(hi[-1]))
    t_down = time.perf_counter() - t0
    ni = args.host_ind; nh = 2 * ni
    t0 = time.perf_counter()
    top = int(hi[511])
    h = unpack(words[:top], nh)
    c = h.sum(axis=1).astype(np.int64)
    n11 = (h[:512] @ h.T).astype(np.int64)
    num = nh * n11 - c[:512, None] * c[None, :]
    den = c * (nh - c)
    q = numpy_q40(num, den[:512, None], den[None, :])
    score = np.array([q[t, lo[t]:hi[t]].sum(dtype=np.uint64) for t in range(512)], dtype=np.uint64)
    terms = np.array([(den[lo[t]:hi[t]] > 0).sum() for t in range(512)], dtype=np.uint64)
    t_prod = time.perf_counter() - t0
    scaled = t_prod * (2 * n) / nh * S / 512
    rec = {"step": "download_scores", "n_ind": n, "n_loci": L, "score_snps": S, "window": w, "download_s": t_down, "bytes_downloaded": int(words.nbytes),
           "products_ind_timed": ni, "products_snps_timed": 512, "products_s_timed": t_prod, "products_s_scaled": scaled, "total_s": t_down + scaled,
           "sha256_host_ind": digest([score, terms])}
    ctx.close()
    print(json.dumps(rec), flush=True)


STEPS = {"counts": step_counts, "scores": step_scores, "download": step_download, "download_scores": step_download_scores}


def run_step(args, step, extra):
    cmd = [sys.executable, os.path.abspath(__file__), str(args.n_ind), str(args.n_loci), "--repeats", str(args.repeats), "--host-ind", str(args.host_ind),
           "--score-snps", str(args.score_snps), "--step", step] + extra
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
    ap.add_argument("--blocks", default="1024,4096,8192")
    ap.add_argument("--score-snps", type=int, default=100_000)
    ap.add_argument("--windows", default="500,1000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-ind", type=int, default=2048)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--block", type=int)
    ap.add_argument("--window", type=int)
    args = ap.parse_args()
    args.host_ind = min(args.host_ind, args.n_ind)
    if args.step:
        STEPS[args.step](args)
        return 0
    ok = True
    for B in (int(v) for v in args.blocks.split(",") if v):
        if 2 * B > args.n_loci:
            print(json.dumps({"block": B, "error": f"two blocks are more than the {args.n_loci} SNPs"}), flush=True)
            return 1
        d = run_step(args, "counts", ["--block", str(B)])
        h = d and run_step(args, "download", ["--block", str(B)])
        if not h:
            return 1
        agree = d["sha256_host_ind"] == h["sha256_host_ind"]
        ok = ok and agree and d["call_median_s"] < h["download_s"]
        print(json.dumps({"summary": "ld_counts_rate", "n_ind": args.n_ind, "n_loci": args.n_loci, "block": B, "device_call_median_s": d["call_median_s"],
                          "device_pair_haplotypes_per_s": d["pair_haplotypes_per_s"], "device_fraction_of_i8_rate": d["fraction_of_i8_rate"],
                          "download_s": h["download_s"], "host_products_s_scaled": h["products_s_scaled"], "download_route_s": h["total_s"],
                          "route_over_device": h["total_s"] / d["call_median_s"], "device_beats_download_alone": d["call_median_s"] < h["download_s"],
                          "counts_agree": agree}), flush=True)
    for w in (int(v) for v in args.windows.split(",") if v):
        d = run_step(args, "scores", ["--window", str(w)])
        h = d and run_step(args, "download_scores", ["--window", str(w)])
        if not h:
            return 1
        agree = d["sha256_host_ind"] == h["sha256_host_ind"]
        ok = ok and agree and d["call_median_s"] < h["download_s"]
        print(json.dumps({"summary": "ld_scores_rate", "n_ind": args.n_ind, "n_loci": args.n_loci, "score_snps": args.score_snps, "window": w,
                          "device_call_median_s": d["call_median_s"], "device_pair_haplotypes_per_s": d["pair_haplotypes_per_s"],
                          "device_fraction_of_i8_rate": d["fraction_of_i8_rate"], "download_s": h["download_s"], "host_products_s_scaled": h["products_s_scaled"],
                          "download_route_s": h["total_s"], "route_over_device": h["total_s"] / d["call_median_s"],
                          "device_beats_download_alone": d["call_median_s"] < h["download_s"], "scores_agree": agree}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
