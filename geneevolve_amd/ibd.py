"""Identity by descent from the device's walk over the ancestry interval lists (GevContext.ibd_sharing / ancestry_bp): the shared
length, segment count and longest segment of every pair of haplotypes, realised coancestry and inbreeding of individuals, and admixture
proportions by root population, summed over chromosomes.  Nothing is downloaded but the integer matrices; every statistic is one
float64 division of exact integers.  segments() lists the IBD segments themselves (GevContext.ibd_segments): where the tracts two
haplotypes share lie on each chromosome.  Works on contexts without genotype planes: the lists are all it reads."""
from collections import namedtuple

import numpy as np

from . import _ranges
from ._ranges import chrs as _chrs, individuals as _individuals, rows as _rows

IBDSharing = namedtuple("IBDSharing", "span_bp shared_bp n_seg max_seg")
IBDSharing.__doc__ = """span_bp: the chromosome's length (last minus first position of its recombination map); shared_bp / n_seg / max_seg:
uint64 / uint32 / uint64 [n_a][n_b] per pair of haplotype rows (row = 2 * individual + chromatid): the summed length, the number and the
longest of the segments of at least min_bp base pairs along which both rows descend from the same founder haplotype"""


def sharing(ctx, pop, chr, a=None, b=None, pop_b=None, min_bp=0):
    """IBDSharing of haplotype rows a of `pop` against rows b of pop_b (None: `pop`) on one chromosome; a, b: None (every row) or (begin, n)"""
    pop_b = pop if pop_b is None else pop_b
    a0, na = _rows(ctx, pop, a); b0, nb = _rows(ctx, pop_b, b)
    return IBDSharing(ctx._span_bp[(pop, chr)], *ctx.ibd_sharing(chr, pop, a0, na, pop_b, b0, nb, min_bp))


def segments_over_chromosomes(chrs, per_chr):
    """one array with a leading `chr` field (int32) from the segment arrays of several chromosomes (GevContext.ibd_segments, each sorted
    by (row_a, row_b, st)), the chromosomes in ascending order: sorted by (chr, row_a, row_b, st)"""
    from .capi import SEGMENT_DTYPE
    return _ranges.segments_over_chromosomes(chrs, per_chr, SEGMENT_DTYPE)


def segments(ctx, pop, chrs=None, rows=None, pop_b=None, rows_b=None, min_bp=0, upper=None):
    """the IBD segments of haplotype rows `rows` of `pop` against rows `rows_b` of pop_b (None: `pop`, and then rows_b None: `rows`
    again) over the chromosomes `chrs` (None: the active ones): a structured array (chr, st, en, row_a, row_b) sorted by
    (chr, row_a, row_b, st), [st, en) half-open, rows absolute in their populations.  upper: only pairs with row_a < row_b; None: True
    when both sides are the same rows of the same population"""
    same_pop = pop_b is None or pop_b == pop
    pop_b = pop if pop_b is None else pop_b
    a0, na = _rows(ctx, pop, rows)
    b0, nb = (a0, na) if same_pop and rows_b is None else _rows(ctx, pop_b, rows_b)
    if upper is None:
        upper = same_pop and (a0, na) == (b0, nb)
    chrs = _chrs(ctx, chrs)
    return segments_over_chromosomes(chrs, [ctx.ibd_segments(k, pop, a0, na, pop_b, b0, nb, min_bp, upper) for k in chrs])


def segment_individuals(seg):
    """(ind_a, chromatid_a, ind_b, chromatid_b) of segment records: row = 2 * individual + chromatid"""
    a, b = np.asarray(seg["row_a"]), np.asarray(seg["row_b"])
    return a >> 1, a & 1, b >> 1, b & 1


def coancestry_from_sums(shared_sum, span_sum):
    """float64 [n][n] from int64 / uint64 [2 n][2 n] shared base pairs per pair of haplotype rows summed over chromosomes, and the sum of the
    chromosomes' spans: entry (i, k) = the four haplotype pairs' sum / (4 span_sum); the integer sums first, one division at the end"""
    s = np.asarray(shared_sum, dtype=np.uint64)
    four = s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]
    return four.astype(np.float64) / np.float64(4 * int(span_sum))


def inbreeding_from_sums(shared_own, span_sum):
    """float64 [n] from the shared base pairs of every individual's own two haplotypes summed over chromosomes / span_sum"""
    return np.asarray(shared_own, dtype=np.uint64).astype(np.float64) / np.float64(int(span_sum))


def admixture_from_sums(bp_sum):
    """float64 [n][n_pop] from uint64 [2 n][n_pop] base pairs by root population per haplotype row summed over chromosomes: an individual's
    two rows added, each column over their total (NaN for an individual whose rows cover nothing)"""
    bp = np.asarray(bp_sum, dtype=np.uint64)
    ind = bp[0::2] + bp[1::2]
    tot = ind.sum(axis=1, dtype=np.uint64).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tot[:, None] > 0, ind.astype(np.float64) / tot[:, None], np.nan)


def coancestry(ctx, pop, ind=None, chrs=None, min_bp=0):
    """float64 [n][n]: the realised coancestry of individuals `ind` (None: everybody, or (begin, n)) of one population: the base pairs
    shared by the four pairs of their haplotypes, summed over the chromosomes `chrs` (None: the active ones), over 4 times the
    chromosomes' summed length.  The diagonal is (1 + F_i) / 2 with F_i of inbreeding()"""
    i0, n = _individuals(ctx, pop, ind)
    total = np.zeros((2 * n, 2 * n), dtype=np.uint64)
    span = 0
    for chr in _chrs(ctx, chrs):
        span += ctx._span_bp[(pop, chr)]
        total += ctx.ibd_sharing(chr, pop, 2 * i0, 2 * n, pop, 2 * i0, 2 * n, min_bp, want=(True, False, False))[0]
    return coancestry_from_sums(total, span)


def inbreeding(ctx, pop, ind=None, chrs=None, min_bp=0):
    """float64 [n]: the realised inbreeding of each individual: the fraction of the chromosomes' length along which its own two
    haplotypes descend from the same founder haplotype"""
    i0, n = _individuals(ctx, pop, ind)
    own = np.zeros(n, dtype=np.uint64)
    span = 0
    blk = 2048                                                  # individuals a diagonal block: 4096 rows a side, one sub-block of the call
    for chr in _chrs(ctx, chrs):
        span += ctx._span_bp[(pop, chr)]
        for j in range(0, n, blk):
            m = min(blk, n - j)
            s = ctx.ibd_sharing(chr, pop, 2 * (i0 + j), 2 * m, pop, 2 * (i0 + j), 2 * m, min_bp, want=(True, False, False))[0]
            own[j:j + m] += s[np.arange(0, 2 * m, 2), np.arange(1, 2 * m, 2)]
    return inbreeding_from_sums(own, span)


def admixture(ctx, pop, chrs=None):
    """float64 [n_people][n_pop]: the fraction of each individual's covered base pairs that descends from founders of each root population"""
    total = np.zeros((2 * ctx.pop_size(pop), ctx.n_pop), dtype=np.uint64)
    for chr in _chrs(ctx, chrs):
        total += ctx.ancestry_bp(pop, chr)[0]
    return admixture_from_sums(total)
