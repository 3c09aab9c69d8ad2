"""gev_dbg_roh_host: the word logic of geneevolve_amd/csrc/gev_roh.h (start and end masks, carries across words, the open start, the
range mask) built for the host, against the per-SNP truth of tests/roh_inputs.py on constructed rows: hets at word, chunk and tile
edges, gapped positions, every parameter set and SNP range, individual sub-ranges, the capacity rule with a guard, the refusals, and the
helpers of geneevolve_amd/roh.py on arrays.  No device.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

from geneevolve_amd import capi, roh
from geneevolve_amd.capi import ROH_SEGMENT_DTYPE
from tests import roh_inputs as R

L = R.L


@pytest.fixture(scope="module")
def built():
    """the constructed individuals: (names, unpacked rows, packed rows, positions, the truth without limits over everything)"""
    patterns = R.het_patterns()
    bits01 = R.rows_from_patterns(patterns)
    pos = R.positions()
    return [name for name, _ in patterns], bits01, capi.pack_rows(bits01), pos, R.truth(bits01, pos)


def host(lib, words, pos, s0=0, ns=None, i0=0, ni=None, **lim):
    return lib.dbg_roh_host(words, L, pos, s0, ns, i0, ni, **lim)


def test_inputs_are_what_the_cases_need(built):
    names, bits01, words, pos, full = built
    assert len(names) == 40 and words.shape == (80, (L + 63) // 64) and L % 64 == 13
    d = np.diff(pos.astype(np.int64))
    assert sorted(np.flatnonzero(d > R.STEP).tolist()) == sorted(R.GAPS_AFTER) and (d[list(R.GAPS_AFTER)] == R.GAP + R.STEP).all()
    assert pos[R.SHARED[0]] == pos[R.SHARED[1]] == pos[R.SHARED[2]] and (d >= 0).all()
    n_roh = full[0]
    assert n_roh[0] == 1 and full[2][0] == L and full[1][0] == int(pos[-1] - pos[0]), "all homozygous: one run of L"
    assert n_roh[1] == 0 and full[3][1] == 0, "all heterozygous: none"
    assert n_roh[2] == L // 64 + 1 and n_roh[3] == L // 64 + 1 and n_roh[4] == 1 and full[2][4] == L - 2
    assert (n_roh[5:20] == 2).all(), "a single het inside the row: two runs"
    R.consistent(full)


def test_constructed_rows_under_every_parameter_set_and_range(gpu_lib, built):
    names, bits01, words, pos, full = built
    sets = R.parameter_sets(full[5])
    at, above = R.truth(bits01, pos, **sets[1]), R.truth(bits01, pos, **sets[2])
    assert len(at[5]) > len(above[5]) > 0, "min_snps is the length of a run"
    at, above = R.truth(bits01, pos, **sets[3]), R.truth(bits01, pos, **sets[4])
    assert len(at[5]) > len(above[5]) > 0, "min_bp is the length of a run"
    assert len(R.truth(bits01, pos, **sets[6])[5]) > len(R.truth(bits01, pos, **sets[5])[5]) == len(full[5]), "one below the gap splits runs, the gap itself none"
    for lim in sets:
        for s0, ns in R.SNP_RANGES:
            want = R.truth(bits01, pos, s0, ns, **lim)
            got = host(gpu_lib, words, pos, s0, ns, **lim)
            R.same(got, want, f"SNPs [{s0},+{ns}) {lim}")
            R.consistent(got)


def test_individual_sub_ranges_and_row_stride(gpu_lib, built):
    names, bits01, words, pos, full = built
    wide = np.full((words.shape[0], words.shape[1] + 3), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    wide[:, :words.shape[1]] = words
    lim = R.parameter_sets(full[5])[7]
    for i0, ni in ((0, 1), (39, 1), (1, 38), (5, 15), (17, 0)):
        for s0, ns in ((0, L), (37, 8192 + 100)):
            want = R.truth(bits01, pos, s0, ns, i0, ni, **lim)
            R.same(host(gpu_lib, words, pos, s0, ns, i0, ni, **lim), want, f"individuals [{i0},+{ni}) SNPs [{s0},+{ns})")
            R.same(host(gpu_lib, wide, pos, s0, ns, i0, ni, **lim), want, f"individuals [{i0},+{ni}) SNPs [{s0},+{ns}), wider rows")
    # outputs that are not wanted
    got = gpu_lib.dbg_roh_host(words, L, pos, want_cover=False, want_list=False)
    assert got[4] is None and got[5] is None
    R.same(got, full, "no cover, no list")
    f = gpu_lib._f("dbg_roh_host")
    q = R.params()
    n_roh = np.zeros(40, dtype=np.uint32); max_bp = np.zeros(40, dtype=np.uint64)
    assert f(words, words.shape[1], 40, L, pos, 0, L, 0, 40, C.byref(q), n_roh, None, None, max_bp, None, None, 0, None) == 0
    assert np.array_equal(n_roh, full[0]) and np.array_equal(max_bp, full[3])


def test_capacity_rule(gpu_lib, built):
    names, bits01, words, pos, full = built
    f = gpu_lib._f("dbg_roh_host")
    for (s0, ns, i0, ni), lim in (((0, L, 0, 40), {}), ((37, 8292, 3, 30), dict(min_snps=60, max_gap_bp=R.GAP))):
        q = R.params(**lim)
        want = R.truth(bits01, pos, s0, ns, i0, ni, **lim)[5]
        R.capacity_cases(lambda out, cap, n: f(words, words.shape[1], 40, L, pos, s0, ns, i0, ni, C.byref(q), None, None, None, None, None, out, cap, n), want)
    q = R.params(min_snps=L + 1)
    rc, n, buf = R.raw(lambda out, cap, n: f(words, words.shape[1], 40, L, pos, 0, L, 0, 40, C.byref(q), None, None, None, None, None, out, cap, n), 4)
    assert rc == 0 and n == 0 and (buf == R.SENTINEL).all(), "a threshold beyond every run"


def test_empty_forms_and_refusals(gpu_lib, built):
    names, bits01, words, pos, full = built
    f = gpu_lib._f("dbg_roh_host")
    q = R.params()
    w = words.shape[1]
    # n_ind == 0: zeros into cover, nothing else; n_snps == 0: zeros into the per-individual vectors
    got = host(gpu_lib, words, pos, 5, 100, 7, 0)
    assert len(got[4]) == 100 and not got[4].any() and len(got[0]) == 0 and len(got[5]) == 0
    got = host(gpu_lib, words, pos, L, 0, 3, 9)
    assert all(len(v) == 9 and not v.any() for v in got[:4]) and len(got[4]) == 0 and len(got[5]) == 0
    out = np.full(4 * ROH_SEGMENT_DTYPE.itemsize, R.SENTINEL, dtype=np.uint8)
    vec = np.full(40, 7, dtype=np.uint32)

    def refused(word, s=(0, L), i=(0, 40), params=True, n_total=True, null_out=False, capacity=4, stride=w):
        n = C.c_uint64(12345)
        rc = f(words, stride, 40, L, pos, s[0], s[1], i[0], i[1], C.byref(q) if params else None, vec, None, None, None, None,
               None if null_out else capi._p(out), capacity, C.byref(n) if n_total else None)
        assert rc == -1 and word in gpu_lib.last_error(), f"{rc} {gpu_lib.last_error()}"
        assert (out == R.SENTINEL).all() and n.value == 12345 and (vec == 7).all()
    refused("SNPs", s=(L - 1, 2))
    refused("SNPs", s=(L + 1, 0))
    refused("individuals", i=(39, 2))
    refused("individuals", i=(41, 0))
    refused("params", params=False)
    refused("null output", null_out=True)
    refused("without n_total", n_total=False)
    refused("words", stride=w - 1)


def test_roh_module_helpers_on_arrays(built):
    names, bits01, words, pos, full = built
    span = int(pos[-1] - pos[0])
    f = roh.f_roh_from_sums(full[1], span)
    assert f.dtype == np.float64 and f[0] == 1.0 and f[1] == 0.0 and (f <= 1.0).all()
    assert np.array_equal(f, full[1].astype(np.float64) / np.float64(span))
    isl = roh.islands_from_cover(full[4], 40)
    assert np.array_equal(isl, full[4].astype(np.float64) / 40.0) and isl.max() <= 39 / 40
    half = R.truth(bits01, pos, 0, 8192)
    s = roh.summary_over_chromosomes([span, 5], [full[:4], half[:4]])
    assert s.span_bp == span + 5 and np.array_equal(s.n_roh, full[0].astype(np.uint64) + half[0]) and np.array_equal(s.roh_bp, full[1] + half[1])
    assert np.array_equal(s.roh_snps, full[2].astype(np.uint64) + half[2]) and np.array_equal(s.max_bp, np.maximum(full[3], half[3]))
    seg = roh.segments_over_chromosomes([2, 0], [full[5], half[5]])
    assert seg.dtype.names == ("chr",) + ROH_SEGMENT_DTYPE.names and seg["chr"].tolist() == [0] * len(half[5]) + [2] * len(full[5])
    assert all(np.array_equal(seg[name][:len(half[5])], half[5][name]) and np.array_equal(seg[name][len(half[5]):], full[5][name]) for name in ROH_SEGMENT_DTYPE.names)
    assert roh._limits(100, 1.5, 0.25) == dict(min_snps=100, min_bp=1500, max_gap_bp=250)


class _FixedSize:
    """what the range helpers ask of a context"""
    def pop_size(self, pop):
        return 30 + pop

    def active_chrs(self):
        return [0, 2]


def test_range_helpers_and_chromosome_order_for_both_record_types():
    from geneevolve_amd import _ranges, ibd, relatedness
    from geneevolve_amd.capi import SEGMENT_DTYPE
    ctx = _FixedSize()
    # the default extent: individuals, or two haplotype rows each
    for helper, per in ((_ranges.individuals, 1), (_ranges.rows, 2)):
        assert helper(ctx, 0, None) == (0, 30 * per) and helper(ctx, 3, None) == (0, 33 * per)
        assert helper(ctx, 0, (4, 7)) == (4, 7) and helper(ctx, 0, np.array([4, 7])) == (4, 7)
        assert helper(ctx, 0, range(5, 12)) == (5, 7) and helper(ctx, 0, slice(None, 9)) == (0, 9) and helper(ctx, 0, slice(3, 9)) == (3, 6)
        assert all(type(v) is int for v in helper(ctx, 0, np.array([4, 7])))
    # the modules' own names are these helpers
    assert ibd._rows is _ranges.rows and ibd._individuals is _ranges.individuals and roh._individuals is _ranges.individuals
    assert relatedness._range is _ranges.individuals
    assert ibd._chrs(ctx, None) == [0, 2] and roh._chrs(ctx, (np.int64(3), 1)) == [3, 1]
    # chromosomes handed over out of order, for both record types
    for module, dtype in ((ibd, SEGMENT_DTYPE), (roh, ROH_SEGMENT_DTYPE)):
        per_chr = []
        for k, n in enumerate((3, 0, 5)):
            a = np.zeros(n, dtype=dtype)
            for j, name in enumerate(dtype.names):
                a[name] = 100 * k + 10 * j + np.arange(n)
            per_chr.append(a)
        got = module.segments_over_chromosomes([7, 4, 1], per_chr)
        assert got.dtype.names == ("chr",) + dtype.names and got["chr"].dtype == np.int32
        assert all(got.dtype.fields[name][0] == dtype.fields[name][0] for name in dtype.names)
        assert got["chr"].tolist() == [1] * 5 + [7] * 3
        assert all(np.array_equal(got[name][:5], per_chr[2][name]) and np.array_equal(got[name][5:], per_chr[0][name]) for name in dtype.names)
        assert np.array_equal(got, _ranges.segments_over_chromosomes([7, 4, 1], per_chr, dtype))
        assert len(module.segments_over_chromosomes([], [])) == 0 and module.segments_over_chromosomes([], []).dtype == got.dtype
