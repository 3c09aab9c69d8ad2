"""The trait-sum arithmetic of geneevolve_amd/csrc/gev_traitsum.h compiled for the host, gev_dbg_trait_sums_host: the masking, the digit
split, the byte order of both operands and the recombination the device kernels run, with a plain integer loop in place of the matrix
instruction, on haplotype-major rows in host memory, against plain numpy -- by equality.  Then geneevolve_amd/assoc.py on host sums
against the exact rational.  No device is needed."""
import decimal
from fractions import Fraction

import numpy as np
import pytest

from geneevolve_amd import assoc, capi
from tests.snp_counts_inputs import random_rows
from tests.test_snp_counts_cpu import padded
from tests.trait_sums_inputs import EDGE_QUANTA, NAMES, Q_MAX, numpy_trait_sums, one_hot_traits, one_hot_value, random_quanta

N_PEOPLE, L = 340, 200
N_IND = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 333)
# (snp_begin, n_snps): 1, 15, 16, 17, 63, 64, 65, 129 SNPs, across the edges of the 64-SNP words of a haplotype row
SNP_RANGES = [(199, 1), (56, 15), (60, 16), (0, 17), (1, 63), (64, 64), (63, 65), (40, 129)]
N_TRAITS = (0, 1, 3, 4, 5, 17)


def ind_ranges(n_ind):
    """ranges of n_ind individuals that begin at the population's first, inside a half word (16 individuals), inside a word (32), inside a
    4-word step (128), behind a whole step, and that end at the population's last"""
    return sorted({(min(b, N_PEOPLE - n_ind), n_ind) for b in (0, 5, 21, 70, 135, N_PEOPLE)})


@pytest.fixture(scope="module")
def population():
    """340 people x 200 SNPs with every allele frequency from 0 to 1: the unpacked rows and the packed ones at a wider stride with garbage
    in the pad words and in the bits of the last word behind L"""
    rs = np.random.RandomState(41)
    bits = random_rows(rs, N_PEOPLE, L)
    wide = padded(capi.pack_rows(bits), 2, rs)
    wide[:, capi.words_for(L) - 1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(L % 64)
    return bits, capi.pack_rows(bits), wide


def check(lib, rows, bits, q, s0, ns, i0, ni, what=""):
    got = lib.dbg_trait_sums_host(rows, L, q, s0, ns, i0, ni)
    want = numpy_trait_sums(bits, s0, ns, i0, ni, q)
    where = f"individuals [{i0},+{ni}), SNPs [{s0},+{ns}), {q.shape[0]} traits {what}"
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == (np.int64 if name.endswith("sum") else np.uint32) and g.shape == w.shape, name + ", " + where
        assert np.array_equal(g, w), name + ", " + where
    return got


@pytest.mark.parametrize("n_ind", N_IND)
def test_host_trait_sums_equal_numpy(gpu_lib, population, n_ind):
    bits, tight, wide = population
    rs = np.random.RandomState(100 + n_ind)
    k = 0
    for i0, ni in ind_ranges(n_ind):
        for s0, ns in SNP_RANGES:
            q = random_quanta(rs, N_TRAITS[k % len(N_TRAITS)], ni); k += 1
            check(gpu_lib, wide, bits, q, s0, ns, i0, ni, "stride + 2 words of garbage")
        check(gpu_lib, tight, bits, random_quanta(rs, 5, ni), 3, 129, i0, ni, "tight rows")


@pytest.mark.parametrize("n_traits", N_TRAITS)
def test_every_number_of_traits_on_every_snp_range(gpu_lib, population, n_traits):
    bits, tight, wide = population
    rs = np.random.RandomState(7 + n_traits)
    for s0, ns in SNP_RANGES + [(0, L)]:
        check(gpu_lib, wide, bits, random_quanta(rs, n_traits, 333), s0, ns, 3, 333)


@pytest.mark.parametrize("i0", [0, 3, 16, 37, 200], ids=lambda b: f"ind_begin {b}")
def test_one_hot_traits_tell_the_byte_order(gpu_lib, population, i0):
    """for every position p of a 128-individual matrix step a trait whose only quantum sits at individual i0 + first + p, a different
    value with four non-zero digits at each: gsum[p][j] = g_pj q_p, so one misplaced byte of the trait operand is one wrong entry.  Even
    and odd first individuals, first words inside and at the start of a step"""
    bits, tight, wide = population
    ni = min(333, N_PEOPLE - i0)
    for first in (0, ni - 128):
        q = one_hot_traits(ni, first)
        gsum, hetsum, het, hom = check(gpu_lib, wide, bits, q, 0, L, i0, ni, f"one-hot from {first}")
        g = bits[2 * (i0 + first):2 * (i0 + first + 128):2, :].astype(np.int64) + bits[2 * (i0 + first) + 1:2 * (i0 + first + 128):2, :]
        vals = np.array([one_hot_value(p) for p in range(128)], dtype=np.int64)
        assert np.array_equal(gsum, g * vals[:, None]) and np.array_equal(hetsum, (g == 1) * vals[:, None])
        assert (g == 1).any(axis=1).all() and (g == 2).any(axis=1).all(), "every position is told apart by some SNP"


def test_digit_carry_edges(gpu_lib, population):
    """quanta at +-2^30, 0, +-1, +-127, +-128, +-129, +-32768 and their like: alone in a trait (one value for everybody), and every edge
    at every position of a word"""
    bits, tight, wide = population
    for i0, ni in ((0, N_PEOPLE), (5, 129)):
        alone = np.repeat(np.array(EDGE_QUANTA, dtype=np.int32)[:, None], ni, axis=1)
        gsum = check(gpu_lib, wide, bits, alone, 10, 70, i0, ni, "one edge value each")[0]
        c = bits[2 * i0:2 * (i0 + ni), 10:80].sum(axis=0, dtype=np.int64)
        assert np.array_equal(gsum, np.array(EDGE_QUANTA, dtype=np.int64)[:, None] * c[None, :])
        rolled = np.stack([np.roll(np.resize(np.array(EDGE_QUANTA, dtype=np.int32), ni), k) for k in range(len(EDGE_QUANTA))])
        check(gpu_lib, wide, bits, rolled, 10, 70, i0, ni, "the edges rolled over the individuals")


def test_nothing_asked_for_and_nulls(gpu_lib, population):
    bits, tight, wide = population
    f = gpu_lib._f("dbg_trait_sums_host")
    q = random_quanta(np.random.RandomState(3), 3, 9)
    want = numpy_trait_sums(bits, 10, 4, 20, 9, q)

    def call(ns, ni, nt, outs, trait=q):
        return f(wide, wide.shape[1], N_PEOPLE, L, 10, ns, 20, ni, trait, nt, *outs)
    mats = [np.full((3, 4), 7, dtype=np.int64) for _ in range(2)]; vecs = [np.full(4, 7, dtype=np.uint32) for _ in range(2)]
    all4 = mats + vecs
    assert call(0, 9, 3, all4) == 0 and all((a == 7).all() for a in mats + vecs), "no SNP: nothing is touched"
    assert call(4, 0, 3, all4, None) == 0 and not any(a.any() for a in mats + vecs), "no individual: zeros"
    for k in range(4):                                       # each output on its own
        out = np.full(want[k].shape, 7, dtype=np.int64 if k < 2 else np.uint32)
        outs = [None] * 4; outs[k] = out
        assert call(4, 9, 3, outs) == 0 and np.array_equal(out, want[k]), NAMES[k]
    for a in vecs:
        a[:] = 7
    assert call(4, 9, 0, [None, None] + vecs, None) == 0, "no trait: the two count vectors only"
    assert np.array_equal(vecs[0], want[2]) and np.array_equal(vecs[1], want[3])


def test_host_trait_sums_refusals(gpu_lib, population):
    bits, tight, wide = population
    q = np.zeros((2, 5), dtype=np.int32)

    def refused(call, word, code=-1):
        with pytest.raises(capi.GevError) as e:
            call()
        assert word in str(e.value) and e.value.code == code, str(e.value)

    refused(lambda: gpu_lib.dbg_trait_sums_host(wide, L, q, L - 1, 2, 0, 5), "SNPs")
    refused(lambda: gpu_lib.dbg_trait_sums_host(wide, L, q, 0, 5, N_PEOPLE - 4, 5), "individuals")
    refused(lambda: gpu_lib.dbg_trait_sums_host(tight[:, :3], L, q, 0, 5, 0, 5), "words")
    for bad in (Q_MAX + 1, -Q_MAX - 1, -(1 << 31)):
        q1 = q.copy(); q1[1, 3] = bad
        refused(lambda: gpu_lib.dbg_trait_sums_host(wide, L, q1, 0, 5, 0, 5), "quantum")
    q1 = q.copy(); q1[0, 0] = Q_MAX; q1[1, 4] = -Q_MAX
    gpu_lib.dbg_trait_sums_host(wide, L, q1, 0, 5, 0, 5)
    f = gpu_lib._f("dbg_trait_sums_host")
    out = np.zeros((2, 5), dtype=np.int64)
    assert f(wide, wide.shape[1], N_PEOPLE, L, 0, 5, 0, 5, None, 2, out, None, None, None) == -1
    assert "null trait" in gpu_lib.last_error()
    big = (1 << 22) + 1
    assert f(None, 0, big, 10, 0, 1, 0, big, None, 1, None, None, None, None) == -5
    assert "at most" in gpu_lib.last_error()


# ---- assoc.py on host sums ---------------------------------------------------------------------------
class HostContext:
    """the call assoc.py makes, answered from rows in host memory by the host build of the trait sums"""

    def __init__(self, lib, bits01):
        self.lib, self.rows, self._nsnp = lib, capi.pack_rows(bits01), {(0, 0): bits01.shape[1]}

    def pop_size(self, pop):
        return self.rows.shape[0] // 2

    def snp_trait_sums(self, pop, chr, trait, snp_begin, n_snps, ind_begin, n_ind):
        return self.lib.dbg_trait_sums_host(self.rows, self._nsnp[(0, 0)], trait, snp_begin, n_snps, ind_begin, n_ind)


def test_quantise_round_trips():
    """|q scale + mean - y| <= scale / 2, decided in exact rationals; the largest deviation maps to +-2^bits"""
    rs = np.random.RandomState(5)
    y = np.stack([rs.normal(170.0, 9.0, 500), rs.standard_cauchy(500) * 1e-3, rs.uniform(-1, 1, 500) * 1e12, np.full(500, 3.25)])
    for bits in (30, 12):
        q, scale, mean = assoc.quantise(y, bits)
        assert q.dtype == np.int32 and q.shape == y.shape and np.abs(q.astype(np.int64)).max() == 1 << bits and not q[3].any() and scale[3] == 1.0
        for t in range(3):
            half = Fraction(float(scale[t])) / 2
            for i in range(500):
                assert abs(int(q[t, i]) * Fraction(float(scale[t])) + Fraction(float(mean[t])) - Fraction(float(y[t, i]))) <= half, (bits, t, i)
    q, scale, mean = assoc.quantise(y[0])
    assert q.shape == (1, 500)


def _dec(fr):
    return decimal.Decimal(fr.numerator) / decimal.Decimal(fr.denominator)


def _exact_stats(g, y):
    """g: list of 0/1/2, y: list of Python integers -> the statistics as decimals of 60 digits from exact rationals (None: undefined)"""
    N = len(g)
    sg, sy = sum(g), sum(y)
    sxx = Fraction(N * sum(a * a for a in g) - sg * sg, N); syy = Fraction(N * sum(b * b for b in y) - sy * sy, N)
    sxy = Fraction(N * sum(a * b for a, b in zip(g, y)) - sg * sy, N)
    beta = sxy / sxx
    sse = syy - sxy * sxy / sxx
    se2 = sse / (N - 2) / sxx
    out = {"beta": _dec(beta), "se": _dec(se2).sqrt(), "t": _dec(beta) / _dec(se2).sqrt(), "r2": _dec(sxy * sxy / (sxx * syy))}
    cls = [[b for a, b in zip(g, y) if a == k] for k in range(3)]
    for k in range(3):
        out[f"mean{k}"] = _dec(Fraction(sum(cls[k]), len(cls[k]))) if cls[k] else None
    present = [c for c in cls if c]
    ssb = sum(Fraction(sum(c) ** 2, len(c)) for c in present) - Fraction(sy * sy, N)
    out["F"] = _dec((ssb / (len(present) - 1)) / ((syy - ssb) / (N - len(present))))
    return out


def _numpy_stats(g, y):
    """the textbook two-pass regression and one-way analysis of variance in float64"""
    g, y = np.asarray(g, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N = len(g)
    dg, dy = g - g.mean(), y - y.mean()
    sxx, syy, sxy = (dg * dg).sum(), (dy * dy).sum(), (dg * dy).sum()
    beta = sxy / sxx
    res = dy - beta * dg
    se = np.sqrt((res * res).sum() / (N - 2) / sxx)
    out = {"beta": beta, "se": se, "t": beta / se, "r2": sxy * sxy / (sxx * syy)}
    present = [k for k in range(3) if (g == k).any()]
    for k in range(3):
        out[f"mean{k}"] = y[g == k].mean() if k in present else None
    ssb = sum((g == k).sum() * (y[g == k].mean() - y.mean()) ** 2 for k in present)
    ssw = sum(((y[g == k] - y[g == k].mean()) ** 2).sum() for k in present)
    out["F"] = (ssb / (len(present) - 1)) / (ssw / (N - len(present)))
    return out


def test_assoc_statistics_against_the_exact_rational(gpu_lib):
    """additive and genotypic on host sums against Python fractions on 6 traits x 50 SNPs (300 pairs) of 300 individuals, SNPs with one,
    two and three carriers and a class of one among them; traits: quanta over the whole +-2^30 with a large common offset (the
    cancelling numerator), and traits that follow a SNP closely.  The bound is what numpy's own float64 two-pass regression and analysis
    of variance miss the exact rational by on the same input; the module forms the cancelling terms in integers and is held to no more.
    Largest relative distances measured (numpy / module): beta 5.0e-14 / 1.0e-16, se 3.0e-14 / 1.3e-16, t 5.0e-14 / 1.5e-16,
    r2 9.9e-14 / 1.1e-16, F 4.7e-9 / 1.1e-16; the class means are one correctly rounded quotient either way (1.1e-16 both)"""
    decimal.getcontext().prec = 60
    rs = np.random.RandomState(17)
    n, ns = 300, 50
    bits = random_rows(rs, n, ns)
    bits[:, 1] = 0; bits[7, 1] = 1                                        # one carrier
    bits[:, 2] = 0; bits[[10, 11, 40], 2] = 1                             # a class of one individual 1/1, one 0/1
    bits[:, 3] = 1; bits[100, 3] = 0                                      # near-monomorphic at the other end
    bits[:, 4] = 0; bits[[20, 33, 250], 4] = 1
    g = (bits[0::2] + bits[1::2]).astype(np.int64)
    q = np.empty((6, n), dtype=np.int64)
    q[0] = rs.randint(-Q_MAX, Q_MAX + 1, n)
    q[1] = (1 << 30) - rs.randint(0, 5000, n)                             # a spread 2^-18 of the offset
    q[2] = -(1 << 29) + rs.randint(-300, 300, n) + 1000 * g[:, 10]
    q[3] = 100000 * g[:, 20] + rs.randint(-3, 4, n)                       # r^2 close to 1
    q[4] = rs.randint(-1, 2, n)
    q[5] = (rs.normal(0, 1, n) * (1 << 26)).astype(np.int64) + (1 << 27) * (g[:, 30] == 1)
    q = np.clip(q, -Q_MAX, Q_MAX).astype(np.int32)
    s = assoc.sums(HostContext(gpu_lib, bits), 0, 0, q)
    assert s.n_ind == n and (s.scale == 1).all() and not s.mean.any()
    assert [int(v) for v in s.sum_q] == [int(v) for v in q.astype(np.int64).sum(axis=1)]
    assert [int(v) for v in s.sum_q2] == [sum(int(v) ** 2 for v in row) for row in q]
    add, gen = assoc.additive(s), assoc.genotypic(s)
    got = {"beta": add.beta, "se": add.se, "t": add.t, "r2": add.r2, "mean0": gen.means[0], "mean1": gen.means[1], "mean2": gen.means[2], "F": gen.F}
    mono = g.min(axis=0) == g.max(axis=0)
    assert mono.any() and (~mono).sum() >= 40
    worst = {k: [0.0, 0.0] for k in got}                                  # per statistic: numpy's largest relative distance, the module's
    pairs = 0
    for j in range(ns):
        if mono[j]:
            for k in ("beta", "se", "t", "r2", "F"):
                assert np.isnan(got[k][:, j]).all(), (k, j)
            continue
        for t in range(6):
            exact, plain = _exact_stats([int(v) for v in g[:, j]], [int(v) for v in q[t]]), _numpy_stats(g[:, j], q[t])
            pairs += 1
            for k, e in exact.items():
                if e is None:
                    assert np.isnan(got[k][t, j]), (k, t, j)
                    continue
                for col, v in enumerate((plain[k], got[k][t, j])):
                    assert np.isfinite(v), (k, t, j, col)
                    d = abs(decimal.Decimal(float(v)) - e) / abs(e) if e else abs(decimal.Decimal(float(v)))
                    worst[k][col] = max(worst[k][col], float(d))
    assert pairs >= 240
    for k, (plain, mine) in worst.items():
        print(f"{k}: numpy {plain:.3g}, assoc {mine:.3g}")
    for k, (plain, mine) in worst.items():
        assert mine <= plain, (k, plain, mine)
    assert (gen.df1 + gen.df2 == n - 1).all() and gen.df1.max() == 2 and gen.df1[1] == 1 and (gen.df1[mono] == 0).all()


def test_assoc_in_the_units_of_y(gpu_lib):
    """a float phenotype is quantised, and the slope and the class means come back in its units: against numpy's regression on the floats
    within the quantisation (scale / 2 per individual) -- here 1e-7 relative is ample and says that scale and mean are applied"""
    rs = np.random.RandomState(23)
    bits = random_rows(rs, 200, 40)
    g = (bits[0::2] + bits[1::2]).astype(np.float64)
    y = np.stack([170.0 + 3.0 * g[:, 5] + rs.normal(0, 2.0, 200), rs.normal(-4.0, 1e-3, 200)])
    s = assoc.sums(HostContext(gpu_lib, bits), 0, 0, y[:, 10:160], snps=(2, 30), ind=(10, 150))
    add, gen = assoc.additive(s), assoc.genotypic(s)
    for t in range(2):
        for j in range(30):
            gj, yt = g[10:160, 2 + j], y[t, 10:160]
            if gj.min() == gj.max():
                assert np.isnan(add.beta[t, j])
                continue
            ref = _numpy_stats(gj, yt)
            assert np.isclose(add.beta[t, j], ref["beta"], rtol=1e-6, atol=1e-9) and np.isclose(add.se[t, j], ref["se"], rtol=1e-6)
            assert np.isclose(add.r2[t, j], ref["r2"], rtol=1e-6, atol=1e-12) and np.isclose(gen.F[t, j], ref["F"], rtol=1e-6, atol=1e-9)
            for k in range(3):
                assert (ref[f"mean{k}"] is None and np.isnan(gen.means[k, t, j])) or np.isclose(gen.means[k, t, j], ref[f"mean{k}"], rtol=1e-8)
