"""CPU checks of the device selection step's interface: the C-ABI declares it, capi binds it (and says so clearly where a library
lacks it), and the host mirror is the reference's formula (Simulation::ras_selection_func, reference src/Simulation.cpp:3386-3428)
with C's semantics: overflow and division by zero give inf or NaN, never an exception."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from geneevolve_amd import capi
from geneevolve_amd.host import ras_selection_func, selection_func
from tests.helpers import c_selection_formula, ulp_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("compute_selection", "download_selection", "get_selection_gen0", "set_selection_gen0", "generation_begin_selected", "random_mate_selected")


def test_header_declares_and_capi_binds_the_selection_entry_points(gpu_lib):
    hdr = open(os.path.join(ROOT, "include", "geneevolve_amd.h")).read()
    declared = set(re.findall(r"\b(gev_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert "gev_" + name in declared and name in capi.ABI_SYMBOLS and gpu_lib.exports(name), name
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define GEV_SEL_([A-Z]+)\s+(\d+)", hdr)}
    assert codes == {"none": 0, "default": 1, "logit": 2, "probit": 3, "stab": 4, "thr": 5}
    assert {k or "default": v for k, v in capi.SELECTION_FUNCS.items()} == codes
    # struct gev_selection_params: int32 gen_num, func; double par1, par2; three pointers
    P = capi.gev_selection_params
    assert C.sizeof(P) == 48 and P.par1.offset == 8 and P.omega.offset == 24 and P.phen_shift.offset == 40
    for m in ("compute_selection", "download_selection", "get_selection_gen0", "set_selection_gen0", "generation_begin_selected", "random_mate_selected"):
        assert callable(getattr(capi.GevContext, m))


def test_a_library_without_the_entry_points_is_refused_clearly(oracle_lib):
    assert not oracle_lib.exports("compute_selection")
    ctx = oracle_lib.create(1, 1, 1)
    with pytest.raises(capi.GevError) as e:
        ctx.compute_selection(0, 0, "none", 0, 0, [1.0], [1.0])
    assert e.value.code == -5 and "does not export" in str(e.value)
    with pytest.raises(capi.GevError):
        ctx.generation_begin_selected(0, 1, 10)
    ctx.close()


def test_host_mirror_default_logit_is_the_reference_formula():
    z = np.array([-3.0, -0.5, 0.0, 1e-3, 0.7, 2.5, 36.0, 709.0, 710.0, 1e4, -1e4])
    got = ras_selection_func(1, "", 0.0, 0.0, z)
    for v, g in zip(z.tolist(), got.tolist()):
        b0, b1 = 0.0, 1.0                             # :3393-3399
        try:
            y = math.exp(b0 + b1 * v)
        except OverflowError:
            y = math.inf                              # C's exp: inf, and inf/(1+inf) is NaN
        want = y / (1 + y)
        assert (math.isnan(want) and math.isnan(g)) or g == want, (v, g, want)
    assert np.isnan(got[z > 709.78]).all() and not np.isnan(got[z <= 709.0]).any()
    # generation 0 and "none": everybody may marry; the other kinds are selection_func, unchanged
    assert np.array_equal(ras_selection_func(0, "logit", 5.0, 5.0, z), np.ones(len(z)))
    assert np.array_equal(ras_selection_func(3, "none", 5.0, 5.0, z), np.ones(len(z)))
    zz = np.linspace(-3, 3, 41)
    for kind, p1, p2 in (("logit", 1.0, 1.0), ("probit", -0.5, 0.8), ("stab", 0.3, 1.5), ("thr", 0.5, 0.2)):
        assert np.array_equal(ras_selection_func(2, kind, p1, p2, zz), selection_func(kind, p1, p2, zz))
    with pytest.raises(NotImplementedError):          # selection_func itself keeps its behaviour
        selection_func("", 0.0, 1.0, zz)


# (kind, p1, p2, z, what the reference's C++ returns under glibc, written out from C's semantics)
C_EDGES = [
    ("logit", 0.0, 1000.0, [1.0], [math.nan]),                # exp(1000) = inf, inf / (1 + inf) = NaN
    ("stab", 0.0, 1e-200, [1.0, 0.0], [0.0, 1 / (math.sqrt(2.0 * 3.1415926) * 1e-200)]),   # pow(1e200, 2) = inf, exp(-inf) = 0; z == mu: exp(0) = 1
    ("probit", 0.0, 0.0, [1.0, 0.0, -2.0], [1.0, math.nan, 0.0]),   # 1/0 = inf, erf(inf) = 1; 0/0 = NaN; -2/0 = -inf, erf(-inf) = -1
    ("stab", 0.0, 0.0, [1.0], [math.nan]),                    # 1/(sqrt(2 pi) * 0) = inf, times exp(-inf) = 0: inf * 0 = NaN
    ("thr", 0.3, 0.5, [0.5, np.nextafter(0.5, 1.0), np.nextafter(0.5, 0.0), math.nan], [0.3, 1.0, 0.3, 1.0]),   # z <= thr gives p1, NaN gives 1
]


@pytest.mark.parametrize("kind,p1,p2,z,want", C_EDGES, ids=["logit-overflow", "stab-tiny-sigma", "probit-zero-sigma", "stab-zero-sigma", "thr-at-threshold"])
def test_host_mirror_follows_c_at_the_edges(kind, p1, p2, z, want):
    got = ras_selection_func(1, kind, p1, p2, np.array(z))
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(got)
    assert np.array_equal(got[ok], np.array(want)[ok]), (got, want)
    if kind != "thr":
        assert ulp_distance(got, c_selection_formula(kind, p1, p2, z)).max() == 0, "the mpmath-rounded C formula gives the same"
    if kind == "logit":
        assert np.isnan(ras_selection_func(1, "", 0.0, 0.0, np.array([1000.0]))[0]), "the default (logit 0 1) overflows the same way"


@pytest.mark.parametrize("kind,p1,p2", [("", 0.0, 0.0), ("logit", 1.0, 1.0), ("logit", -2.0, 3.5), ("probit", -0.3, 0.8), ("stab", 0.2, 1.3), ("stab", -0.1, 0.05)])
def test_host_mirror_is_within_glibc_of_the_correctly_rounded_formula(kind, p1, p2):
    """the mirror (glibc libm) against c_selection_formula (libm calls correctly rounded with mpmath, + - * / rounded to double)
    over z in [-40, 40]: logit within 2 ulps (exp's ulp, through y/(1+y)); probit within 2**-53 absolute (1 + erf cancels in the
    lower tail, so its ulp is erf's ulp near 1); stab within 2 ulps per unit of |exp's argument| (glibc's pow(x, 2) is within an
    ulp, not always correctly rounded, and exp multiplies that by its argument)"""
    z = np.linspace(-40.0, 40.0, 20001)
    got, want = ras_selection_func(1, kind, p1, p2, z), c_selection_formula(kind, p1, p2, z)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if kind == "probit":
        assert np.max(np.abs(got - want)) <= 2.0 ** -53
    elif kind == "stab":
        arg = 0.5 * ((z - p1) / p2) ** 2
        assert np.max(ulp_distance(got, want) / np.maximum(1.0, arg)) <= 2.0
    else:
        assert ulp_distance(got, want).max() <= 2
