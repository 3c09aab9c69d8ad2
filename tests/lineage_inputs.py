"""Inputs and the truth of the lineage tests (test_lineage_cpu.py, test_gpu_lineage.py).  The truth is a linear scan per (row, position)
for the part with st <= x < en, in Python integers: no bisection, no cursor, nothing shared with geneevolve_amd/csrc/gev_lineage.h."""
from fractions import Fraction

import numpy as np

from geneevolve_amd.capi import LINEAGE_SITE_DTYPE, NO_FOUNDER

OUTPUTS = ("fid", "counts", "site", "pop_counts")


def rows_of(parts, off):
    """[[(st, en, hap_index, root_population)]] per haplotype row, Python integers, from (parts, offsets) as download_intervals returns them"""
    st, en, hap, rp = (parts[k].tolist() for k in ("st", "en", "hap_index", "root_population"))
    return [[(st[q], en[q], hap[q], rp[q]) for q in range(int(off[r]), int(off[r + 1]))] for r in range(len(off) - 1)]


def covering(row, x):
    """(hap_index, root_population) of the part of the row that covers x, or None"""
    for st, en, hap, rp in row:
        if st <= x < en:
            return hap, rp
    return None


def bases(n_founder_haps):
    nfh = [int(x) for x in n_founder_haps]
    return [sum(nfh[:p]) for p in range(len(nfh) + 1)]


def truth(rows, pos, n_founder_haps, want_counts=True):
    """{fid uint32 [n_pos][n_rows], counts uint32 [n_pos][F] (None unless wanted), site [n_pos], pop_counts uint32 [n_pos][n_pop]} of the
    rows (as rows_of gives them) at the positions (Python integers, any order)"""
    base = bases(n_founder_haps)
    n_pop, F = len(base) - 1, base[-1]
    fid = np.full((len(pos), len(rows)), NO_FOUNDER, dtype=np.uint32)
    counts = np.zeros((len(pos), F), dtype=np.uint32) if want_counts else None
    site = np.zeros(len(pos), dtype=LINEAGE_SITE_DTYPE)
    pop_counts = np.zeros((len(pos), n_pop), dtype=np.uint32)
    for p, x in enumerate(pos):
        x = int(x)
        per = {}
        for r, row in enumerate(rows):
            cov = covering(row, x)
            if cov is None:
                continue
            hap, rp = cov
            assert 0 <= rp < n_pop and hap < base[rp + 1] - base[rp]
            f = base[rp] + hap
            fid[p, r] = f
            per[f] = per.get(f, 0) + 1
            pop_counts[p, rp] += 1
        if want_counts:
            for f, k in per.items():
                counts[p, f] = k
        top = max(per.values(), default=0)
        site[p] = (sum(k * k for k in per.values()), sum(per.values()), len(per), top, min((f for f, k in per.items() if k == top), default=NO_FOUNDER))
    return {"fid": fid, "counts": counts, "site": site, "pop_counts": pop_counts}


def from_fid(fid, n_founder_haps, want_counts=True):
    """the truth's counts, site and pop_counts from a founder-id matrix [n_pos][n_rows], by counting (np.bincount per position; the top
    founder is the first index of the largest count)"""
    base = bases(n_founder_haps)
    n_pop, F = len(base) - 1, base[-1]
    counts = np.zeros((len(fid), F), dtype=np.uint32)
    for p in range(len(fid)):
        ids = fid[p][fid[p] != NO_FOUNDER]
        assert len(ids) == 0 or int(ids.max()) < F
        counts[p] = np.bincount(ids, minlength=F)
    site = np.zeros(len(fid), dtype=LINEAGE_SITE_DTYPE)
    site["sum_sq"] = (counts.astype(np.uint64) ** 2).sum(axis=1, dtype=np.uint64)
    site["n_covered"] = counts.sum(axis=1, dtype=np.uint64)
    site["n_lineages"] = (counts != 0).sum(axis=1)
    site["top_count"] = counts.max(axis=1) if F else 0
    site["top_founder"] = np.where(site["n_covered"] > 0, counts.argmax(axis=1) if F else 0, NO_FOUNDER)
    pop_counts = np.stack([counts[:, base[q]:base[q + 1]].sum(axis=1, dtype=np.uint64) for q in range(n_pop)], axis=1).astype(np.uint32)
    return {"fid": fid, "counts": counts if want_counts else None, "site": site, "pop_counts": pop_counts}


def truth_scan(parts, off, pos, n_founder_haps, want_counts=True):
    """truth() for populations too large for a Python loop per (row, position): still a linear scan -- every part of every row in turn
    marks the positions with st <= x < en -- but one part against all positions at a time, as exact uint64 comparisons; the rest by
    from_fid.  test_lineage_cpu.py holds it equal to truth(), positions around 2^63 and at 2^64 - 1 included"""
    base = bases(n_founder_haps)
    pos = np.ascontiguousarray(pos, dtype=np.uint64)
    st, en, hap, rp = (parts[k] for k in ("st", "en", "hap_index", "root_population"))
    fid = np.full((len(pos), len(off) - 1), NO_FOUNDER, dtype=np.uint32)
    for r in range(len(off) - 1):
        for q in range(int(off[r]), int(off[r + 1])):
            hit = (st[q] <= pos) & (pos < en[q])
            assert (fid[hit, r] == NO_FOUNDER).all(), "the parts of a row must not overlap"
            assert 0 <= int(rp[q]) < len(base) - 1 and int(hap[q]) < base[int(rp[q]) + 1] - base[int(rp[q])]
            fid[hit, r] = base[int(rp[q])] + int(hap[q])
    return from_fid(fid, n_founder_haps, want_counts)


def ties(counts_or_truth_rows):
    """per position: how many founders share the top count (0 where nothing is covered), from a counts matrix"""
    c = np.asarray(counts_or_truth_rows)
    top = c.max(axis=1) if c.shape[1] else np.zeros(len(c), dtype=c.dtype)
    return np.where(top > 0, (c == top[:, None]).sum(axis=1), 0)


def boundary_positions(rows, extra=()):
    """every part boundary and its two neighbours inside [0, 2^64), sorted, with `extra` mixed in"""
    out = set(int(x) for x in extra)
    for row in rows:
        for st, en, _, _ in row:
            for b in (st, en):
                out.update(x for x in (b - 1, b, b + 1) if 0 <= x < 1 << 64)
    return sorted(out)


def same(got, want, what, names=OUTPUTS):
    """the named outputs of a call (a dict or a tuple in OUTPUTS' order, None = not asked for) equal the truth's, dtype, shape and bytes"""
    if not isinstance(got, dict):
        got = dict(zip(names, got))
    for name in names:
        g, w = got.get(name), want[name]
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)[:5].tolist()
            raise AssertionError(f"{what}: {name} differs at {bad}: got {[g[tuple(b)] for b in bad]}, expected {[w[tuple(b)] for b in bad]}")


def fge_fraction(site_row):
    n, s = int(site_row["n_covered"]), int(site_row["sum_sq"])
    return Fraction(n * n, s) if s else None


def ibd_fraction(site_row):
    n, s = int(site_row["n_covered"]), int(site_row["sum_sq"])
    return Fraction(s - n, n * (n - 1)) if n >= 2 else None
