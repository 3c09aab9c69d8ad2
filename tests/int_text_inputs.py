"""Inputs of the .int interval file tests (test_int_text_cpu.py, test_gpu_int_text.py): the files the fixtures record, the founder
names of tests/cli_inputs.py, and a plain Python statement of Simulation::ras_write_hap_to_interval_format (src/Simulation.cpp:1582-1639)."""
import hashlib
import re

import numpy as np

from geneevolve_amd.capi import PART_DTYPE

HEADER = b"h_ID chr hap st en hap_index gen0_indv root_pop\n"
# every fixture that records .int files; ex1full records no parts at its last generation and is left out
FIXTURES = ("am1", "am2", "c4mini", "dense", "ex1mut", "ex1sub", "gam2", "mig2", "mig3c", "om1", "sel1", "syn1k", "vc1", "vcf1", "vt2")
N_RECORDED_FILES = 71
U64 = 1 << 64


def founder_names(fx):
    """the .indv ids tests/cli_inputs.py:61-63 writes: p{root_pop}i{k+1}, one list per root population"""
    return [[f"p{ip}i{k + 1}" for k in range(int(fx[f"pop{ip}_n_founder_hap"]) // 2)] for ip in range(int(fx["n_pop"]))]


def recorded_files(fx):
    """-> [(sha key, generation, pop, chr, prefix of the recorded state arrays, chr label)] for every .int file the fixture records"""
    out = []
    for k in sorted(fx):
        m = re.fullmatch(r"intfile_(?:g(\d+)_)?pop(\d+)_chr(\d+)_sha", k)
        if not m:
            continue
        g = int(m.group(1)) if m.group(1) else int(fx["n_gen"])
        ip, ic = int(m.group(2)), int(m.group(3))
        pre = f"g{g}_pop{ip}_postmig_" if f"g{g}_pop{ip}_postmig_ids" in fx else f"g{g}_pop{ip}_"
        out.append((k, g, ip, ic, pre, int(fx[f"pop{ip}_chr{ic}_label"])))
    return out


def parts_of(rows):
    """[st, en, hap_index, root_pop] rows -> gev_part records"""
    rows = np.asarray(rows).reshape(-1, 4)
    p = np.zeros(len(rows), dtype=PART_DTYPE)
    p["st"], p["en"], p["hap_index"], p["root_population"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    return p


def sha256(b):
    return np.frombuffer(hashlib.sha256(b).digest(), dtype=np.uint8)


def py_text(parts, off, ids, label, names, header=True, ind_begin=0, n_ind=None):
    """the file's bytes with Python's own str(); the reference's unsigned arithmetic (ID + 1 and hap_index + 1 wrap at 2^64)"""
    n_ind = len(ids) - ind_begin if n_ind is None else n_ind
    out = [HEADER] if header else []
    for ih in range(ind_begin, ind_begin + n_ind):
        for ihap in range(2):
            for q in range(int(off[2 * ih + ihap]), int(off[2 * ih + ihap + 1])):
                p = parts[q]
                h, rp = int(p["hap_index"]), int(p["root_population"])
                out.append(f"{(int(ids[ih]) + 1) % U64} {label} {ihap} {int(p['st'])} {int(p['en'])} {(h + 1) % U64} {names[rp][h // 2]}.{1 + (h & 1)} {rp + 1}\n".encode())
    return b"".join(out)
