"""Python handle on the CPU oracle (oracle/libgev_oracle.so, symbols gevo_*).

TEST INFRASTRUCTURE ONLY: importable from tests/, __graft_entry__.smoke() and the
cpu_baseline leg of bench.py -- never from geneevolve_amd/.
It reuses the product's generic ctypes binding class (same ABI table, other prefix).
"""
import os
import subprocess

import numpy as np

from geneevolve_amd.capi import PART_DTYPE, GevLibrary

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "libgev_oracle.so")

# the known-answer helpers gev_oracle.cpp exports beside the ABI, in the form of capi.ABI (tests hold both equal to its definitions)
KAT_ABI = {
    "kat_rand": "void: u32 int int*",
    "kat_minstd": "void: u32 int u64*",
    "kat_u01": "void: u32 int f64*",
    "kat_uint": "void: u32 u64 u64 int u64*",
    "kat_normal": "void: u32 f64 int f64*",
    "kat_canonical": "f64: u64 u64",
    "kat_sim_loc_rec": "int: u64* f64* size u64 u32 u64* size int*",
    "kat_recombine": "int: part* u64* u64* u64* int u64* size part* u64* u64* size size",
}


def build(force=False):
    src = os.path.join(_HERE, "gev_oracle.cpp")
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(src):
        subprocess.run(["make", "-C", _HERE, "libgev_oracle.so"], check=True, stdout=subprocess.DEVNULL)
    return LIB


def load():
    return GevLibrary(build(), prefix="gevo_", extra_abi=KAT_ABI)


# known-answer helpers -----------------------------------------------------------------------
def kat_rand(lib, seed, n):
    out = np.zeros(n, dtype=np.int32)
    lib._f("kat_rand")(seed, n, out)
    return out


def kat_minstd(lib, seed, n):
    out = np.zeros(n, dtype=np.uint64)
    lib._f("kat_minstd")(seed, n, out)
    return out


def kat_u01(lib, seed, n):
    out = np.zeros(n, dtype=np.float64)
    lib._f("kat_u01")(seed, n, out)
    return out


def kat_uint(lib, engine_seed, lo, hi, n):
    out = np.zeros(n, dtype=np.uint64)
    lib._f("kat_uint")(engine_seed, lo, hi, n, out)
    return out


def kat_normal(lib, seed, sd, n):
    out = np.zeros(n, dtype=np.float64)
    lib._f("kat_normal")(seed, sd, n, out)
    return out


def kat_canonical(lib, x1, x2):
    return lib._f("kat_canonical")(x1, x2)


def kat_sim_loc_rec(lib, bp, prob, bp_dist, seed, cap=4096):
    bp = np.ascontiguousarray(bp, dtype=np.uint64); prob = np.ascontiguousarray(prob, dtype=np.float64)
    locs = np.zeros(cap, dtype=np.uint64); nx = np.zeros(2, dtype=np.int32)
    n = lib._f("kat_sim_loc_rec")(bp, prob, len(bp), int(bp_dist), seed, locs, cap, nx)
    return locs[:n].copy(), nx


def kat_recombine(lib, parts, mut_counts, muts, hap_n, start, locs):
    parts = np.ascontiguousarray(parts, dtype=PART_DTYPE)
    mc = np.ascontiguousarray(mut_counts, dtype=np.uint64); mu = np.ascontiguousarray(muts, dtype=np.uint64)
    hn = np.ascontiguousarray(hap_n, dtype=np.uint64); lc = np.ascontiguousarray(locs, dtype=np.uint64)
    cap_p, cap_m = 4 * (len(parts) + len(lc)) + 16, 4 * len(mu) + 16
    op = np.zeros(cap_p, dtype=PART_DTYPE); omc = np.zeros(cap_p, dtype=np.uint64); om = np.zeros(cap_m, dtype=np.uint64)
    n = lib._f("kat_recombine")(parts, mc, mu, hn, start, lc, len(lc), op, omc, om, cap_p, cap_m)
    return op[:n].copy(), omc[:n].copy(), om[:int(omc[:n].sum())].copy()
