"""Generations/s of the closed loop with family effects (vc > 0), parental effects (vf > 0) and a selection function, done two ways, at
BASELINE config 2's shape (100k individuals x 1M SNPs, one chromosome), two phenotypes, logit 1 1 every generation.  Prints one JSON line.

  host   : the couples are downloaded with gev_generation_end, the host keeps the pedigree (host.Pedigree), draws the family effects
           (Simulation.common_sibling), keeps last generation's phenotypes and gathers them by ID_Father / ID_Mother
           (host.parental_inputs), and calls gev_scale_ad_compute_gef per phenotype with the three arrays; with --mating am the [n][5]
           pedigree goes up with every gev_generation_begin_assort_selected
  device : gev_set_track_pedigree; gev_generation_phenotypes / gev_phenotypes_result / gev_save_prev_gen: no per-individual array
           crosses the boundary inside the loop (the sexes gev_generation_end returns apart)

Both mate on the device's selection values (gev_compute_selection, enqueued only).  Both modes live in one process, each with its own
context and the same inputs, and take turns: --warmup generations each, then --repeats windows of --steps generations per mode,
alternating, every window closed by gev_sync.  Generation 0's variances of A and D are the host's (comm_var) in both modes, so the two
runs differ only by the rounding of parallel sums: the couples of one further generation are hashed per mode (equal hashes = the same
run) and the largest relative difference of the final phenotypes is reported.

--info host|device: the device mode alone, producing the generation's .info text (Population::ras_save_human_info: the one file the
reference writes every generation) behind every phenotype step, two ways:
  host   : the pedigree, components and selection values are downloaded and formatted by C snprintf on up to 8 threads
           (tools/info_format_host.cpp, what the bound command-line program does)
  device : gev_format_info_text
Windows without and with the file's write (one write per generation, to a temporary directory) alternate; the texts of one further
generation are hashed.  --info none (the default) is the comparison described above, unchanged."""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SCHEMES = [(0.4, 0.0, 0.1, 0.4, 0.1), (0.5, 0.0, 0.2, 0.2, 0.1)]          # va, vd, vc, ve, vf
OMEGA, LAMBDA = [1.0, 0.5], [1.0, 1.0]


class Run:
    def __init__(self, mode, args):
        from geneevolve_amd.capi import GevLibrary
        from geneevolve_amd.host import Simulation, SyntheticConfig, comm_var
        self.mode, self.args, self.device = mode, args, mode == "device"
        cfg = SyntheticConfig(args.n_ind, args.n_loci, n_cv=args.n_cv, nphen=2, seed=12345)
        self.ctx = ctx = GevLibrary().create(1, 1, 2)
        cfg.apply_static(ctx)
        ctx.synth_founders(0, 0, 2 * args.n_ind, 1000)
        for p in range(2):
            ctx.synth_cv_founders(0, p, 0, 2 * args.n_ind, 2000 + p)
        if args.mating == "am":                             # Poisson family sizes: the population's size moves by a few hundred around --n-ind; without
            ctx.reserve(0, args.n_ind + args.n_ind // 20 + 1024)   # room reserved every record size regrows the 25 GB row pool (seconds), in either mode
        if args.mating == "rm" and not args.no_chain:
            ctx.set_generation_chain(2)                     # one ras_glob_seed() per phenotype between two generations (:3078)
        self.sim = sim = Simulation(ctx, 4242, 1, True, track_pedigree=not self.device, device_pedigree=self.device)
        sim.ras_initial_human_gen0(0, args.n_ind)
        add, dom, _, _ = ctx.compute_ad(0, per_chr=False)
        self.s2 = [(comm_var(add[:, p]), comm_var(dom[:, p])) for p in range(2)]
        self.beta = [1.0, 1.0]
        self.g = 0
        self.t_enqueue = []                                 # host time inside gev_generation_phenotypes
        self.t_host_parts = {"common_sibling": 0.0, "gather": 0.0, "gef_calls": 0.0}
        self.t_generation_calls = 0.0                       # host time inside the generation's call pair (mating, reproduce, A/D; the host pedigree in host mode)
        self.phenotypes(first=True)
        ctx.compute_selection(0, 0, "none", 0, 0, OMEGA, LAMBDA, want=())

    def schemes(self):
        return [s + (self.beta[p],) for p, s in enumerate(SCHEMES)]

    def phenotypes(self, first=False):
        ctx, sim, g = self.ctx, self.sim, self.g
        if self.device:
            if first:
                for p in range(2):
                    ctx.set_ad_gen0(0, p, *self.s2[p])
            t0 = time.perf_counter()
            sim.generation_phenotypes(0, g, self.schemes())
            self.t_enqueue.append(time.perf_counter() - t0)
            if g > 0:
                ctx.compute_selection(0, g, "logit", 1.0, 1.0, OMEGA, LAMBDA, want=())
            r = sim.phenotypes_result(0)
            if first:
                self.beta = [float(np.sqrt(SCHEMES[p][4] / (2 * r["var"][p][6]))) for p in range(2)]
            sim.save_prev_gen(0)
            return
        from geneevolve_amd.host import NormalEngine, comm_var, parental_inputs
        n = ctx.pop_size(0)
        t0 = time.perf_counter()
        if first:
            common = [NormalEngine(int(sim.ras_glob_seed()[0])).draw(n, float(np.sqrt(s[2]))) for s in SCHEMES]
        else:
            common = sim.common_sibling(0, [s[2] for s in SCHEMES])
        t1 = time.perf_counter()
        par = [parental_inputs(self.prev[p], sim.ped[0]) for p in range(2)] if not first else [np.zeros((n, 2))] * 2
        t2 = time.perf_counter()
        outs = []
        for p, (va, vd, vc, ve, vf) in enumerate(SCHEMES):
            seed = int(sim.ras_glob_seed()[0])
            outs.append(ctx.scale_ad_compute_gef(0, p, g, seed, va, vd, ve, vf, self.beta[p], self.s2[p][0], self.s2[p][1], common_sibling=common[p],
                                                 f_father=par[p][:, 0], f_mother=par[p][:, 1]))
        t3 = time.perf_counter()
        if not first:
            self.t_host_parts["common_sibling"] += t1 - t0; self.t_host_parts["gather"] += t2 - t1; self.t_host_parts["gef_calls"] += t3 - t2
            ctx.compute_selection(0, g, "logit", 1.0, 1.0, OMEGA, LAMBDA, want=())
        else:
            self.beta = [float(np.sqrt(SCHEMES[p][4] / (2 * comm_var(outs[p]["phen"])))) for p in range(2)]
        self.prev = [o["phen"] for o in outs]
        self.last = outs

    # ---- --info: the generation's .info text
    info_mode, info_path, t_info, n_info, last_text = None, None, 0.0, 0, b""

    def info_text(self):
        ctx = self.ctx
        if self.info_mode == "device":
            return ctx.format_info_text(0)
        n = ctx.pop_size(0)
        ids = ctx.download_pedigree(0)
        comps = [ctx.download_phenotypes(0, p) for p in range(2)]
        sel = ctx.download_selection(0)
        cols = [np.ascontiguousarray(c[k]) for c in comps for k in ("additive", "dominance", "bv", "common_sibling", "e_noise", "parental_effect", "phen")]
        cols += [sel["mating_value"], sel["selection_value"], sel["selection_value_func"]]
        ptrs = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
        if getattr(self, "_fmt", None) is None:
            self._fmt = ctypes.CDLL(os.path.join(ROOT, "tools", "libinfo_format_host.so")).info_format_host
            self._buf = np.empty(n * ctx.info_row_bytes() * 2, dtype=np.uint8)
            self._hdr = ctx.format_info_text(0, 0, 0)
        nb = ctypes.c_size_t()
        sex = np.ascontiguousarray(self.sim.sex[0])
        rc = self._fmt(ctypes.c_void_p(ids.ctypes.data), ctypes.c_void_p(sex.ctypes.data), ptrs, ctypes.c_int(len(cols)), ctypes.c_size_t(n), ctypes.c_int(8),
                       ctypes.c_void_p(self._buf.ctypes.data), ctypes.c_size_t(len(self._buf)), ctypes.byref(nb))
        assert rc == 0
        return self._hdr + self._buf[:nb.value].tobytes()

    def info_step(self):
        t0 = time.perf_counter()
        self.last_text = self.info_text()
        if self.info_path:
            with open(self.info_path, "wb") as f:
                f.write(self.last_text)
        self.t_info += time.perf_counter() - t0; self.n_info += 1

    def generation(self, want_couples=False):
        a, sim = self.args, self.sim
        self.g += 1
        want = want_couples or not self.device               # the host's pedigree and family effects need the couples
        t0 = time.perf_counter()
        if a.mating == "rm":
            sim.next_generation_rm_selected(0, a.n_ind, want_couples=want)
        else:
            sim.next_generation_am_selected(0, a.n_ind, 0.3, 0.1, True, "p", want_couples=want)
        self.t_generation_calls += time.perf_counter() - t0
        self.phenotypes()
        if self.info_mode:
            self.info_step()

    def window(self, steps):
        t0 = time.perf_counter()
        for _ in range(steps):
            self.generation()
        self.ctx.sync()
        return time.perf_counter() - t0

    def step_ms(self):
        """wall time of one phenotype step between two gev_sync (device mode): enqueue + device work + the result's wait"""
        self.g += 1
        if self.args.mating == "rm":
            self.sim.next_generation_rm_selected(0, self.args.n_ind)
        else:
            self.sim.next_generation_am_selected(0, self.args.n_ind, 0.3, 0.1, True, "p")
        self.ctx.sync()
        t0 = time.perf_counter()
        self.phenotypes()
        self.ctx.sync()
        return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--n-ind", type=int, default=100_000)
    ap.add_argument("--n-loci", type=int, default=1_000_000)
    ap.add_argument("--n-cv", type=int, default=1000)
    ap.add_argument("--mating", choices=["rm", "am"], default="rm")
    ap.add_argument("--no-chain", action="store_true", help="no head start across generations (random mating)")
    ap.add_argument("--info", choices=["none", "host", "device"], default="none", help="also produce every generation's .info text, on the host or on the device")
    args = ap.parse_args()
    if args.info != "none":
        return main_info(args)
    out = {"tool": "phenotype_loop_bench", "n_ind": args.n_ind, "n_loci": args.n_loci, "nphen": 2, "mating": args.mating,
           "avoid_inbreeding": args.mating == "am", "selection_function": "logit 1 1", "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    runs = {m: Run(m, args) for m in ("host", "device")}
    for r in runs.values():
        r.window(args.warmup)
    secs = {m: [] for m in runs}
    for _ in range(args.repeats):
        for m, r in runs.items():
            secs[m].append(r.window(args.steps))
    for m, r in runs.items():
        out[m] = {"generations_per_s": [round(args.steps / s, 2) for s in secs[m]], "ms_per_generation": [round(s / args.steps * 1e3, 3) for s in secs[m]]}
    n_timed = args.steps * args.repeats
    out["host"]["host_ms_per_generation"] = {k: round(v / (n_timed + args.warmup) * 1e3, 3) for k, v in runs["host"].t_host_parts.items()}
    for m, r in runs.items():
        out[m]["host_ms_inside_generation_calls"] = round(r.t_generation_calls / (n_timed + args.warmup) * 1e3, 3)
    enq = np.array(runs["device"].t_enqueue[1 + args.warmup:])
    out["device"]["host_ms_inside_generation_phenotypes_median"] = round(float(np.median(enq)) * 1e3, 4)
    out["device"]["phenotype_step_ms_between_syncs"] = round(runs["device"].step_ms(), 3)
    runs["host"].generation()                                # (the host mode makes the generation the device mode's step_ms made)
    hashes, final = {}, {}
    for m, r in runs.items():
        r.generation(want_couples=True)
        hashes[m] = hashlib.sha256(np.ascontiguousarray(r.sim.couples[0]).tobytes()).hexdigest()[:16]
        final[m] = [r.ctx.download_phenotypes(0, p)["phen"] for p in range(2)] if r.device else [o["phen"] for o in r.last]
        out[m]["couples_sha256"] = hashes[m]
        out[m]["glob_state_after"] = int(r.sim.glob.x)
    out["same_couples"] = hashes["host"] == hashes["device"]
    out["final_phenotypes_max_rel_diff"] = float(max(np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-300)) for a, b in zip(final["host"], final["device"])))
    out["device_over_host"] = round(float(np.mean(out["device"]["generations_per_s"]) / np.mean(out["host"]["generations_per_s"])), 3)
    for r in runs.values():
        r.ctx.close()
    print(json.dumps(out))


def main_info(args):
    out = {"tool": "phenotype_loop_bench", "info": args.info, "n_ind": args.n_ind, "n_loci": args.n_loci, "nphen": 2, "mating": args.mating,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats}
    r = Run("device", args)
    r.info_mode = args.info
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "info.pop1.txt")
        r.window(args.warmup)
        secs = {"write_excluded": [], "write_included": []}
        info_ms = {"write_excluded": [], "write_included": []}
        for _ in range(args.repeats):
            for key, p in (("write_excluded", None), ("write_included", path)):
                r.info_path, r.t_info, r.n_info = p, 0.0, 0
                secs[key].append(r.window(args.steps))
                info_ms[key].append(round(r.t_info / r.n_info * 1e3, 3))
        r.info_path = None
        r.generation()
    for key in secs:
        out[key] = {"generations_per_s": [round(args.steps / s, 2) for s in secs[key]], "ms_per_generation": [round(s / args.steps * 1e3, 3) for s in secs[key]],
                    "info_ms_per_generation": info_ms[key]}
    out["text_bytes"] = len(r.last_text)
    out["text_sha256"] = hashlib.sha256(r.last_text).hexdigest()[:16]
    out["glob_state_after"] = int(r.sim.glob.x)
    r.ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
