"""Seconds to produce one .int interval file (Simulation::ras_write_hap_to_interval_format) of a population two ways, at ages at which
the lists have grown (a haplotype gains about one part per generation on BASELINE config 2's map).  Prints one JSON line.

  host   : gev_download_intervals (the whole CSR list) + C snprintf on up to 8 threads (tools/int_format_host.cpp)
  device : gev_format_interval_text

One context breeds by random mating to each generation of --gens in turn; there the two ways take turns, --repeats times each, without
and with the file's write (to a temporary directory).  Both fill buffers allocated beforehand; the texts are compared once per
generation (SHA-256).  The number of SNPs does not enter the file and is kept small."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ind", type=int, default=100_000)
    ap.add_argument("--n-loci", type=int, default=4096)
    ap.add_argument("--gens", default="10,100,300")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--chr-label", type=int, default=22)
    args = ap.parse_args()
    from geneevolve_amd import capi
    from geneevolve_amd.host import Simulation, SyntheticConfig
    hostlib = C.CDLL(os.path.join(ROOT, "tools", "libint_format_host.so"))
    n = args.n_ind
    cfg = SyntheticConfig(n, args.n_loci, n_cv=64, seed=12345, with_mutation=False)
    lib = capi.GevLibrary()
    ctx = lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    ctx.synth_founders(0, 0, 2 * n, 1000); ctx.synth_cv_founders(0, 0, 0, 2 * n, 2000)
    names = [f"p0i{k + 1}" for k in range(n)]
    arena, offs = capi.pack_names(names)
    ctx.set_founder_names(0, names)
    sim = Simulation(ctx, 4242, 1, False, device_pedigree=True)
    sim.ras_initial_human_gen0(0, n)
    nb_, no_ = (C.c_void_p * 1)(arena.ctypes.data), (C.c_void_p * 1)(offs.ctypes.data)
    ids = np.arange(n, dtype=np.int64)                       # Human::ID of a generation = the position (:2473)
    fmt = lib._f("format_interval_text")
    tmp = tempfile.mkdtemp(prefix="int_text_bench_")
    out, g = {"n_individuals": n, "threads": args.threads, "repeats": args.repeats, "generations": {}}, 0
    for target in [int(x) for x in args.gens.split(",")]:
        while g < target:
            sim.next_generation_rm(0, n); g += 1
        ctx.sync()
        size = ctx.interval_text_size(0, 0, args.chr_label, header=False)
        n_parts = C.c_size_t()
        ctx._call("download_intervals", 0, 0, None, None, C.byref(n_parts))
        parts = np.zeros(n_parts.value, dtype=capi.PART_DTYPE); off = np.zeros(2 * n + 1, dtype=np.uint64)
        buf_h, buf_d = np.empty(size, dtype=np.uint8), np.empty(size, dtype=np.uint8)
        nb = C.c_size_t()

        def host(write):
            t0 = time.perf_counter()
            ctx._call("download_intervals", 0, 0, parts, off, C.byref(n_parts))
            t1 = time.perf_counter()
            p = lambda a: a.ctypes.data_as(C.c_void_p)               # (the host formatter is a library of its own, bound without types)
            rc = hostlib.int_format_host(p(parts), p(off), p(ids), C.c_size_t(n), C.c_int(args.chr_label), nb_, no_, C.c_int(args.threads), p(buf_h), C.c_size_t(size), C.byref(nb))
            assert rc == 0 and nb.value == size
            t2 = time.perf_counter()
            if write:
                with open(os.path.join(tmp, "h.int"), "wb") as f:
                    f.write(memoryview(buf_h))
            return {"total": time.perf_counter() - t0, "download": t1 - t0, "format": t2 - t1}

        def device(write):
            t0 = time.perf_counter()
            lib.check(fmt(ctx.h, 0, 0, args.chr_label, 0, n, 0, None, buf_d, size, C.byref(nb)))
            assert nb.value == size
            if write:
                with open(os.path.join(tmp, "d.int"), "wb") as f:
                    f.write(memoryview(buf_d))
            return {"total": time.perf_counter() - t0}

        rec = {"parts": int(n_parts.value), "text_bytes": int(size), "list_bytes": int(n_parts.value) * 32}
        for write in (False, True):
            runs = {"host": [], "device": []}
            for _ in range(args.repeats):
                runs["host"].append(host(write)); runs["device"].append(device(write))
            rec["with_write" if write else "no_write"] = {k: {f: sorted(r[f] for r in v) for f in v[0]} for k, v in runs.items()}
        rec["texts_equal"] = hashlib.sha256(memoryview(buf_h)).digest() == hashlib.sha256(memoryview(buf_d)).digest()
        out["generations"][str(target)] = rec
        print(json.dumps({"generation": target, **rec}), file=sys.stderr, flush=True)       # (the result line comes last, on stdout)
        del parts, buf_h, buf_d
    for f in os.listdir(tmp):
        os.unlink(os.path.join(tmp, f))
    os.rmdir(tmp)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
