"""Founder lineages along the genome from the device's per-position reading of the ancestry interval lists (GevContext.founder_at /
founder_counts): which founder haplotype every haplotype descends from at given positions, local-ancestry dosages per individual, and
per position the ancestry frequencies, the number of founder lineages still alive, the founder-genome equivalents and the probability
that two haplotypes are identical by descent there.  Nothing is downloaded but the integer results; every statistic is one float64
division of exact integers, NaN where the denominator is 0.  Positions may come in any order: they are sorted for the device and the
results returned in the caller's order.  Works on contexts without genotype planes: the lists are all it reads."""
import numpy as np

from ._ranges import individuals as _individuals, rows as _rows
from .capi import NO_FOUNDER

NO_HAP = np.uint64(0xFFFFFFFFFFFFFFFF)


def _sorted_positions(pos):
    """(the positions in non-decreasing order as uint64, inverse) with sorted[inverse] = the caller's order"""
    pos = np.ascontiguousarray(pos, dtype=np.uint64).ravel()
    order = np.argsort(pos, kind="stable")
    inverse = np.empty(len(pos), dtype=np.int64)
    inverse[order] = np.arange(len(pos))
    return np.ascontiguousarray(pos[order]), inverse


def labels(fid, n_founder_haps):
    """(root_population int32, hap_index uint64) of founder ids, -1 / 2^64 - 1 where uncovered (NO_FOUNDER); n_founder_haps: the founder
    haplotypes per root population the ids were made with"""
    fid = np.asarray(fid, dtype=np.uint32)
    ends = np.cumsum(np.asarray(n_founder_haps, dtype=np.uint64), dtype=np.uint64)
    base = np.r_[np.uint64(0), ends[:-1]].astype(np.uint64)
    covered = fid != NO_FOUNDER
    rp = np.searchsorted(ends, fid.astype(np.uint64), side="right").astype(np.int32)
    rp = np.where(covered, rp, np.int32(-1)).astype(np.int32)
    hap = np.where(covered, fid.astype(np.uint64) - base[np.clip(rp, 0, len(base) - 1)], NO_HAP).astype(np.uint64)
    return rp, hap


def at(ctx, pop, chr, pos, rows=None, n_founder_haps=None):
    """uint32 [n_pos][n_rows]: the founder id of every haplotype row of `rows` (None: all, or (begin, n)) at every position, in the
    caller's order of positions; NO_FOUNDER where no part covers the position.  labels() splits an id again"""
    r0, n = _rows(ctx, pop, rows)
    spos, inverse = _sorted_positions(pos)
    return ctx.founder_at(pop, chr, spos, r0, n, n_founder_haps)[inverse]


def local_ancestry(ctx, pop, chr, pos, ind=None, n_founder_haps=None):
    """uint8 [n_ind][n_pos][n_pop]: for every individual of `ind` (None: everybody, or (begin, n)) and position, how many of its two
    haplotypes descend from each root population there (a dosage of 0, 1 or 2; an uncovered haplotype adds to no column)"""
    i0, n = _individuals(ctx, pop, ind)
    nfh = ctx.founder_haps(n_founder_haps)
    rp, _ = labels(at(ctx, pop, chr, pos, (2 * i0, 2 * n), nfh), nfh)                       # [n_pos][2 n]
    hot = rp[:, :, None] == np.arange(ctx.n_pop, dtype=np.int32)[None, None, :]            # [n_pos][2 n][n_pop]
    dosage = hot[:, 0::2, :].astype(np.uint8) + hot[:, 1::2, :].astype(np.uint8)
    return np.ascontiguousarray(dosage.transpose(1, 0, 2))


def sites(ctx, pop, chr, pos, rows=None, n_founder_haps=None):
    """(site LINEAGE_SITE_DTYPE [n_pos], pop_counts uint32 [n_pos][n_pop]) over the haplotype rows of `rows`, in the caller's order of
    positions: per position sum_sq, n_covered, n_lineages, top_count, top_founder, and the rows by root population"""
    r0, n = _rows(ctx, pop, rows)
    spos, inverse = _sorted_positions(pos)
    _, site, pop_counts = ctx.founder_counts(pop, chr, spos, r0, n, n_founder_haps, want=("site", "pop_counts"))
    return site[inverse], pop_counts[inverse]


def _ratio(num, den):
    """num / den in float64, NaN where den == 0; both exactly representable or rounded once each"""
    num = np.asarray(num).astype(np.float64); den = np.asarray(den).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


def ancestry_frequency(site, pop_counts):
    """float64 [n_pos][n_pop]: pop_counts / n_covered, the share of the covered haplotypes that descends from each root population"""
    return _ratio(np.asarray(pop_counts, dtype=np.uint64), np.asarray(site["n_covered"], dtype=np.uint64)[:, None])


def founder_genome_equivalents(site):
    """float64 [n_pos]: n_covered^2 / sum_sq, the number of equally represented founders that would give the position's IBD probability"""
    n = np.asarray(site["n_covered"], dtype=np.uint64)
    return _ratio(n * n, np.asarray(site["sum_sq"], dtype=np.uint64))


def ibd_probability(site):
    """float64 [n_pos]: (sum_sq - n) / (n (n - 1)) with n = n_covered: the probability that two distinct covered haplotypes descend from
    the same founder haplotype at the position (NaN for n < 2)"""
    n = np.asarray(site["n_covered"], dtype=np.uint64)
    return _ratio(np.asarray(site["sum_sq"], dtype=np.uint64) - n, n * (n - np.minimum(n, np.uint64(1))))
