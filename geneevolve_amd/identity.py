"""Identity states per pair of individuals from the device's four-cursor walk over the ancestry interval lists
(GevContext.identity_states): the base pairs along which the four haplotypes of two individuals are in each of Jacquard's nine
condensed identity states, summed over chromosomes, and what a family design reads off them: the state coefficients, kinship,
IBD0 / IBD1 / IBD2, the fraternity (dominance) coefficient and the inbreeding of either side.  Nothing is downloaded but the integer
planes; every statistic is one float64 division of exact integers, NaN where the four haplotypes are nowhere covered together.  Works
on contexts without genotype planes: the lists are all it reads.

Plane s - 1 holds state s (a = the first individual, b = the second):
  1 all four IBD                      4 a autozygous, nothing shared       7 both of a's haplotypes IBD with b's, pairwise
  2 each autozygous, not shared       5 b autozygous, shared with a        8 exactly one pair across
  3 a autozygous, shared with b       6 b autozygous, nothing shared       9 nothing shared"""
import numpy as np

from ._ranges import chrs as _chrs, individuals as _individuals


def states(ctx, pop, chrs=None, ind=None, pop_b=None, ind_b=None):
    """uint64 [9][n_a][n_b]: the base pairs in each identity state of individuals `ind` of `pop` (None: everybody, or (begin, n)) against
    individuals `ind_b` of pop_b (None: `pop`, and then ind_b None: `ind` again), summed over the chromosomes `chrs` (None: the active
    ones)"""
    same_pop = pop_b is None or pop_b == pop
    pop_b = pop if pop_b is None else pop_b
    a0, na = _individuals(ctx, pop, ind)
    b0, nb = (a0, na) if same_pop and ind_b is None else _individuals(ctx, pop_b, ind_b)
    total = np.zeros((9, na, nb), dtype=np.uint64)
    for chr in _chrs(ctx, chrs):
        total += ctx.identity_states(chr, pop, a0, na, pop_b, b0, nb)
    return total


def _over_sum(num, D):
    """num / the sum of the nine planes in float64, NaN where that sum is 0"""
    den = np.asarray(D, dtype=np.uint64).sum(axis=0, dtype=np.uint64).astype(np.float64)
    num = np.asarray(num, dtype=np.uint64).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


def _planes(D):
    D = np.asarray(D, dtype=np.uint64)
    assert D.shape[0] == 9, f"nine planes, {D.shape} given"
    return D


def jacquard(D):
    """float64 [9][...]: the nine condensed identity coefficients, each plane over the sum of the nine"""
    D = _planes(D)
    return _over_sum(D, D)


def kinship(D):
    """float64 [...]: (4 D1 + 2 (D3 + D5 + D7) + D8) / (4 sum): the probability that a random haplotype of a and a random one of b are
    IBD, averaged along the covered length.  An individual against itself gives (1 + F) / 2"""
    D = _planes(D)
    four = np.uint64(4)
    return _over_sum(four * D[0] + np.uint64(2) * (D[2] + D[4] + D[6]) + D[7], D * four)


def ibd012(D):
    """(k0, k1, k2), float64 [...] each: the shares of the covered length along which the two individuals share 0, 1 or 2 haplotypes
    IBD: (D2 + D4 + D6 + D9, D3 + D5 + D8, D1 + D7) / sum"""
    D = _planes(D)
    return _over_sum(D[1] + D[3] + D[5] + D[8], D), _over_sum(D[2] + D[4] + D[7], D), _over_sum(D[0] + D[6], D)


def fraternity(D):
    """float64 [...]: k2 = (D1 + D7) / sum, the coefficient of the dominance variance between the two individuals"""
    return ibd012(D)[2]


def inbreeding(D):
    """(F_a, F_b), float64 [...] each: the share of the covered length along which a's (b's) own two haplotypes are IBD:
    (D1 + D2 + D3 + D4, D1 + D2 + D5 + D6) / sum"""
    D = _planes(D)
    return _over_sum(D[0] + D[1] + D[2] + D[3], D), _over_sum(D[0] + D[1] + D[4] + D[5], D)
