"""The library's %g (geneevolve_amd/csrc/gev_fmt_g.h) compiled for the host, against the C library's snprintf: byte equality on the
edge cases, random bit patterns and the doubles a table-based fast path cannot decide; the share of values on the exact path."""
import numpy as np

from tests import info_text_inputs as I

# values of N(0,1) that took the exact path in the first run of this test: 0 of 262144 (the undecided band is 8 * 2^-64 wide)
NORMAL_EXACT_MEASURED = 0


def host_g(gpu_lib, x):
    out, n_exact = gpu_lib.dbg_format_g_host(x)
    return I.strings(out), n_exact


def test_edge_list_against_glibc(gpu_lib):
    vals = I.EDGES + [-v for v in I.EDGES]
    got, _ = host_g(gpu_lib, vals)
    for v, g in zip(vals, got):
        assert g == I.glibc_g(v), f"{v!r}: {g!r} vs glibc {I.glibc_g(v)!r}"
    for v, want in I.EDGES_STATED.items():
        assert got[vals.index(v)] == want
    assert got[vals.index(I.NAN_NEG)] == b"-nan" and got[vals.index(I.NAN_POS)] == b"nan"
    assert max(len(g) for g in got) <= 13


def test_random_bit_patterns_against_glibc(gpu_lib):
    x = I.random_patterns()
    got, _ = host_g(gpu_lib, x)
    want = I.expected(x)
    bad = [(v, g, w) for v, g, w in zip(x.tolist(), got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(x)} differ, first: {bad[:3]}"
    sub = x[(np.abs(x) < I.DBL_MIN) & (x != 0)]
    assert len(sub) > 50                                             # subnormals are in the set
    assert max(len(g) for g in got) <= 13


def test_near_midpoints_take_the_exact_path(gpu_lib):
    x = I.near_midpoints()
    got, n_exact = host_g(gpu_lib, x)
    want = I.expected(x)
    bad = [(v, g, w) for v, g, w in zip(x.tolist(), got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(x)} differ, first: {bad[:3]}"
    print(f"near-midpoint set: {n_exact} of {len(x)} values took the exact path")
    assert n_exact > 0


def test_share_of_ordinary_values_on_the_exact_path(gpu_lib):
    x = I.normals()
    got, n_exact = host_g(gpu_lib, x)
    assert got == I.expected(x)
    print(f"N(0,1): {n_exact} of {len(x)} values took the exact path")
    assert n_exact <= 10 * NORMAL_EXACT_MEASURED
