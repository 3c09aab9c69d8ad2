"""What the analysis modules (ibd, roh, relatedness) share in reading their arguments: ranges of individuals or haplotype rows, the
chromosomes of a request, and the record lists of several chromosomes joined into one."""
import numpy as np


def individuals(ctx, pop, r, per_individual=1):
    """(begin, n) of a range given as None (everybody), (begin, n) or a range / slice-like with .start and .stop"""
    if r is None:
        return 0, per_individual * ctx.pop_size(pop)
    if hasattr(r, "start"):
        return int(r.start or 0), int(r.stop) - int(r.start or 0)
    return int(r[0]), int(r[1])


def rows(ctx, pop, r):
    """(begin, n) of a range of haplotype rows (two per individual), given as individuals() takes a range"""
    return individuals(ctx, pop, r, 2)


def chrs(ctx, which):
    """the chromosomes of a request: None (the active ones) or a sequence of indices"""
    return list(ctx.active_chrs()) if which is None else [int(k) for k in which]


def segments_over_chromosomes(chrs, per_chr, dtype):
    """one array with a leading `chr` field (int32) from the record arrays (of `dtype`, each in its call's order) of several chromosomes,
    the chromosomes in ascending order"""
    dt = np.dtype([("chr", np.int32)] + [(name, dtype.fields[name][0]) for name in dtype.names])
    order = sorted(range(len(chrs)), key=lambda k: int(chrs[k]))
    out = np.zeros(sum(len(s) for s in per_chr), dtype=dt)
    at = 0
    for k in order:
        part = out[at:at + len(per_chr[k])]
        part["chr"] = int(chrs[k])
        for name in dtype.names:
            part[name] = per_chr[k][name]
        at += len(part)
    return out
