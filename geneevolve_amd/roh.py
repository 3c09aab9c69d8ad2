"""Runs of homozygosity from the device's scan of the haplotype rows (GevContext.roh_summary / roh_segments): per individual the number,
summed length, summed SNPs and the longest of its runs, F_ROH over chromosomes, the runs themselves as one list, and ROH islands (the
share of individuals with a SNP inside a run).  The observed side of ibd.inbreeding: a run is a stretch of consecutive SNPs at which an
individual's two haplotypes carry the same allele (mutations applied), with no allowance for heterozygous calls -- PLINK's --homozyg with
--homozyg-window-het 0, without its sliding window.  Nothing is downloaded but the integer vectors; every statistic is one float64
division of exact integers.  Limits are given in SNPs and kilobases (1 kb = 1000 bp), 0 = none."""
from collections import namedtuple

import numpy as np

from . import _ranges
from ._ranges import chrs as _chrs, individuals as _individuals

ROHSummary = namedtuple("ROHSummary", "span_bp n_roh roh_bp roh_snps max_bp")
ROHSummary.__doc__ = """span_bp: the summed pos[L-1] - pos[0] of the chromosomes; n_roh / roh_bp / roh_snps / max_bp: uint64 [n_ind] per
individual over its qualifying runs on those chromosomes: their number, their summed length in base pairs (last minus first SNP position
of each run), their summed SNPs, and the longest in base pairs (0 without a run)"""


def _limits(min_snps, min_kb, max_gap_kb):
    """the keyword arguments of the context calls from limits in SNPs and kilobases"""
    return dict(min_snps=int(min_snps), min_bp=int(round(min_kb * 1000)), max_gap_bp=int(round(max_gap_kb * 1000)))


def summary_over_chromosomes(spans, per_chr):
    """ROHSummary from the chromosomes' spans and their (n_roh, roh_bp, roh_snps, max_bp, ...) tuples as GevContext.roh_summary returns
    them: integer sums, the longest by maximum"""
    n = len(per_chr[0][0]) if per_chr else 0
    tot = [np.zeros(n, dtype=np.uint64) for _ in range(4)]
    for r in per_chr:
        for k in range(3):
            tot[k] += np.asarray(r[k], dtype=np.uint64)
        tot[3] = np.maximum(tot[3], np.asarray(r[3], dtype=np.uint64))
    return ROHSummary(int(sum(int(s) for s in spans)), *tot)


def f_roh_from_sums(roh_bp, span_bp):
    """float64 [n]: the summed length of every individual's runs over the chromosomes' summed span (NaN for a span of 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(roh_bp, dtype=np.uint64).astype(np.float64) / np.float64(int(span_bp))


def islands_from_cover(cover, n_ind):
    """float64 [n_snps]: the share of the n_ind individuals with each SNP inside a qualifying run"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(cover, dtype=np.uint32).astype(np.float64) / np.float64(int(n_ind))


def segments_over_chromosomes(chrs, per_chr):
    """one array with a leading `chr` field (int32) from the run arrays of several chromosomes (GevContext.roh_segments, each sorted by
    (ind, snp_first)), the chromosomes in ascending order: sorted by (chr, ind, snp_first)"""
    from .capi import ROH_SEGMENT_DTYPE
    return _ranges.segments_over_chromosomes(chrs, per_chr, ROH_SEGMENT_DTYPE)


def summary(ctx, pop, chrs=None, ind=None, min_snps=0, min_kb=0, max_gap_kb=0):
    """ROHSummary of individuals `ind` (None: everybody, or (begin, n)) of one population over the chromosomes `chrs` (None: the active
    ones), each chromosome's whole SNP range"""
    i0, n = _individuals(ctx, pop, ind)
    chrs = _chrs(ctx, chrs)
    lim = _limits(min_snps, min_kb, max_gap_kb)
    return summary_over_chromosomes([ctx._snp_span_bp[(pop, k)] for k in chrs],
                                    [ctx.roh_summary(pop, k, ind_begin=i0, n_ind=n, want_cover=False, **lim) for k in chrs])


def f_roh(ctx, pop, chrs=None, ind=None, min_snps=0, min_kb=0, max_gap_kb=0):
    """float64 [n]: F_ROH of each individual: the summed length of its qualifying runs over the chromosomes, divided by the chromosomes'
    summed pos[L-1] - pos[0]"""
    s = summary(ctx, pop, chrs, ind, min_snps, min_kb, max_gap_kb)
    return f_roh_from_sums(s.roh_bp, s.span_bp)


def segments(ctx, pop, chrs=None, ind=None, min_snps=0, min_kb=0, max_gap_kb=0):
    """the qualifying runs of individuals `ind` over the chromosomes `chrs` (None: the active ones): a structured array (chr, st, en, ind,
    snp_first, n_snps, reserved) sorted by (chr, ind, snp_first); st and en are the positions of the run's first and last SNP"""
    i0, n = _individuals(ctx, pop, ind)
    chrs = _chrs(ctx, chrs)
    lim = _limits(min_snps, min_kb, max_gap_kb)
    return segments_over_chromosomes(chrs, [ctx.roh_segments(pop, k, ind_begin=i0, n_ind=n, **lim) for k in chrs])


def islands(ctx, pop, chr, ind=None, snp_begin=0, n_snps=None, min_snps=0, min_kb=0, max_gap_kb=0):
    """float64 [n_snps]: for each SNP of the range of one chromosome, the share of the individuals `ind` that have it inside a qualifying
    run (cover / n_ind).  Runs are cut at the range's ends"""
    i0, n = _individuals(ctx, pop, ind)
    cover = ctx.roh_summary(pop, chr, snp_begin, n_snps, i0, n, **_limits(min_snps, min_kb, max_gap_kb))[4]
    return islands_from_cover(cover, n)
