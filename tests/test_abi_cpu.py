"""CPU tests of the product library's host side: it loads without a GPU, exports every symbol of
include/geneevolve_amd.h, refuses to compute without a device (no fallback), and its host-built
RNG tables / integer Bernoulli thresholds agree with the oracle's exact arithmetic."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from geneevolve_amd import capi
from oracle import oracle_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


HEADER = os.path.join(ROOT, "include", "geneevolve_amd.h")
ORACLE_SRC = os.path.join(ROOT, "oracle", "gev_oracle.cpp")

# C type names -> the codes of capi.ABI (the oracle spells the handle Ctx and uint32_t by value `unsigned`)
_BASE = {"int": "int", "size_t": "size", "uint32_t": "u32", "unsigned": "u32", "uint64_t": "u64", "unsigned long long": "ull",
         "int64_t": "i64", "int32_t": "i32", "double": "f64", "float": "f32", "char": "u8", "uint8_t": "u8", "void": "void",
         "gev_ctx": "ctx", "Ctx": "ctx"}
_BY_VALUE = {"int", "size", "u32", "u64", "f64"}
_DECL = re.compile(r"(unsigned\s+long\s+long|unsigned|[A-Za-z_]\w*)\s*((?:\*\s*)*)(\w+)?\s*(\[\d*\])?")


def _c_kind(decl, structs):
    """one C parameter or return declaration -> its code in capi.ABI; anything it cannot classify raises"""
    m = _DECL.fullmatch(re.sub(r"\bconst\b", " ", decl).strip())
    assert m, f"cannot parse the declaration {decl!r}"
    base = re.sub(r"\s+", " ", m.group(1))
    stars = m.group(2).count("*") + (1 if m.group(4) else 0)                # (a parameter `T x[n]` is a T*)
    s = re.fullmatch(r"gevo?_(\w+)", base)
    code = _BASE.get(base) or (s.group(1) if s and s.group(1) in structs else None)
    assert code, f"unknown type in {decl!r}"
    assert stars or code in _BY_VALUE | {"void"}, f"{decl!r}: this type is not passed by value"
    return code + "*" * stars


def _c_prototypes(text, prefix, end, structs):
    """{name: "return: parameters"} in capi.ABI's form for every `prefix` function that C text declares (end ";") or defines (end "{")
    at the start of a line"""
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    out = {}
    for m in re.finditer(r"^([A-Za-z_][\w \t]*?[\s*]+)(%s\w+)\s*\(([^()]*)\)\s*%s" % (prefix, re.escape(end)), text, flags=re.M):
        ret = _c_kind(m.group(1), structs)
        params = m.group(3).strip()
        kinds = [] if params in ("", "void") else [_c_kind(p, structs) for p in params.split(",")]
        name = m.group(2)[len(prefix):]
        assert name not in out, f"{prefix}{name} found twice"
        out[name] = " ".join(["str:" if ret == "u8*" else ret + ":"] + kinds)
    return out


def _header():
    """(text, the names followed by a parenthesis, the struct names) of the header"""
    hdr = open(HEADER).read()
    declared = set(re.findall(r"\b(gev_[a-z0-9_]+)\s*\(", hdr)) - {"gev_ctx"}
    structs = set(re.findall(r"typedef\s+struct\s+gev_(\w+)\s*\{", hdr))
    return hdr, declared, structs


def test_header_symbols_all_exported(gpu_lib):
    hdr, declared, structs = _header()
    assert len(declared) >= 30
    for name in sorted(declared):
        assert gpu_lib.exports(name[len("gev_"):]), f"{name} declared in the header but not exported"
    assert declared == {"gev_" + s for s in capi.ABI}, "capi.ABI out of sync with the header"
    protos = _c_prototypes(hdr, "gev_", ";", structs)
    assert {"gev_" + s for s in protos} == declared, "a declaration of the header the prototype parser did not read"
    assert len(protos) >= 119, len(protos)
    for name, shape in protos.items():
        assert capi.ABI[name] == shape, f"capi.ABI[{name!r}] differs from the header's gev_{name}"
    assert list(capi.ABI) == list(protos) and capi.ABI_SYMBOLS == list(capi.ABI)        # (the table follows the header's order)


def test_oracle_definitions_match_the_tables():
    hdr, _, structs = _header()
    src = open(ORACLE_SRC).read()
    defs = _c_prototypes(src, "gevo_", "{", structs)
    # every function the source defines: a name at the start of a line's declarator, whatever the parser made of it
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", src, flags=re.S))
    defined = set(re.findall(r"^[A-Za-z_][\w \t*]*?\b(gevo_\w+)\s*\(", text, flags=re.M))
    assert defined == {"gevo_" + n for n in defs} and len(defs) >= 50, defined ^ {"gevo_" + n for n in defs}
    kat = {n: s for n, s in defs.items() if n.startswith("kat_")}
    assert kat == oracle_api.KAT_ABI
    shared = {n: s for n, s in defs.items() if n not in kat}
    assert len(shared) >= 42 and set(shared) <= set(capi.ABI)
    for name, shape in shared.items():
        want = capi.ABI[name]
        if name == "create":                                               # the oracle has no device to choose
            ret, kinds = want.split(":")
            kinds = kinds.split()
            assert kinds[1] == "int"
            want = " ".join([ret + ":", kinds[0]] + kinds[2:])
        assert shape == want, f"gevo_{name} differs from capi.ABI[{name!r}]"


def test_size_argument_arrives_whole(gpu_lib):
    """plain integers reach a size_t parameter as 64 bits (untyped, ctypes passed 2**32 as the C int 0 and the call returned GEV_OK)"""
    assert gpu_lib._f("dbg_snp_counts_host")(None, 1, 0, 64, 2**32, 0, None, None) == -1
    assert "4294967296" in gpu_lib.last_error()


def test_pointer_parameters_are_typed(gpu_lib):
    f = gpu_lib._f("dbg_snp_counts_host")
    bits = np.zeros((4, 2), dtype=np.uint64)
    het = np.zeros(64, dtype=np.uint32); hom = np.zeros(64, dtype=np.uint32)
    assert f(bits, 2, 2, 64, 0, 64, het, hom) == 0
    # the spelling of raw calls from before the binding was typed stays valid: by-value wrappers, arrays through capi._p
    z = capi.C.c_size_t; het[:] = 7
    assert f(capi._p(bits), z(2), z(2), z(64), z(0), z(64), capi._p(het), capi._p(hom)) == 0 and not het.any(), gpu_lib.last_error()
    assert capi._p(None) is None
    for bad in ((bits.astype(np.float64), het), (bits[:, ::2], het), (bits, het.astype(np.float64))):
        hom[:] = 7
        with pytest.raises(TypeError, match=r"gev_dbg_snp_counts_host: argument [17]"):
            f(bad[0], 2, 2, 64, 0, 64, bad[1], hom)
        assert (hom == 7).all()                                            # refused before the call
    # char* takes uint8, unsigned long long* takes uint64
    out = np.zeros((2, 16), dtype=np.uint8); n = np.zeros(1, dtype=np.uint64)
    assert gpu_lib._f("dbg_format_g_host")(np.array([0.5, 3.0]), 2, out, n) == 0
    assert out[0].tobytes().rstrip(b"\0") == b"0.5" and out[1].tobytes().rstrip(b"\0") == b"3"
    with pytest.raises(TypeError, match="argument 4"):
        gpu_lib._f("dbg_format_g_host")(np.array([0.5]), 1, out, n.astype(np.uint32))
    # a pointer to pointers takes a ctypes array, not a numpy one
    with pytest.raises(TypeError, match="argument 6"):
        gpu_lib._f("dbg_format_interval_text_host")(None, None, 0, None, 1, np.zeros(1, dtype=np.uint64), None, None, 0, 1, None, 0, None)


def test_missing_symbol_is_a_gev_error(oracle_lib):
    missing = [name for name in capi.ABI if not oracle_lib.exports(name)]
    assert len(missing) >= 70
    for name in missing:
        with pytest.raises(capi.GevError) as e:
            oracle_lib._f(name)
        assert e.value.code == -5 and f"does not export gevo_{name}" in str(e.value)


def test_argument_count_is_checked(oracle_lib):
    ctx = oracle_lib.create(1, 1, 1)
    assert ctx.pop_size(0) == 0
    with pytest.raises(TypeError, match="gevo_pop_size takes 3 arguments"):
        ctx._call("pop_size", 0, C.byref(C.c_size_t()), 0)
    with pytest.raises(TypeError, match="gevo_pop_size takes 3 arguments"):
        ctx._call("pop_size", 0)
    ctx.close()


def test_no_cpu_fallback_without_device(gpu_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(capi.GevError) as e:
        gpu_lib.create(1, 1, 1)
    assert e.value.code == -3 and "no CPU fallback" in str(e.value)


def test_threshold_tables_match_exact_canonical(gpu_lib, oracle_lib):
    thr = gpu_lib._f("dbg_threshold")
    can = gpu_lib._f("dbg_canonical")
    rs = np.random.RandomState(7)
    NMAX = 2147483646
    probs = [0.0, 1.0, 5e-4, 0.002, 1e-8, 0.5, 0.999999, 1e-300, 2.0, -1.0, 4.6566128752457969e-10, 1.0 / 3] + list(rs.uniform(0, 1, 40)) + list(10 ** rs.uniform(-9, -1, 40))
    for p in probs:
        out = (C.c_uint32 * 4)()
        assert thr(p, out) == 0
        a_lo, a_hi, b0, b1 = [int(x) for x in out]
        assert a_hi - a_lo <= 2

        def hit_thr(a, b):
            if a < a_lo:
                return True
            if a >= a_hi:
                return False
            return b < (b0 if a == a_lo else b1)
        # probe the whole neighbourhood of the window plus random digits
        cand_a = {0, 1, NMAX - 1, max(a_lo - 1, 0), a_lo, min(a_lo + 1, NMAX - 1), min(a_hi, NMAX - 1), min(a_hi + 1, NMAX - 1)} | {int(x) for x in rs.randint(0, NMAX, 6)}
        for a in cand_a:
            if a >= NMAX:
                continue
            cand_b = {0, 1, NMAX - 1, b0, max(b0 - 1, 0), min(b0 + 1, NMAX - 1), b1, max(b1 - 1, 0), min(b1 + 1, NMAX - 1)} | {int(x) for x in rs.randint(0, NMAX, 6)}
            for b in cand_b:
                if b >= NMAX:
                    continue
                r = oracle_api.kat_canonical(oracle_lib, b + 1, a + 1)      # oracle takes engine outputs x1 (low), x2 (high)
                assert can(a, b) == r
                assert hit_thr(a, b) == (r < p), (p, a, b)


def test_glibc_linear_tables_reproduce_rand(gpu_lib, oracle_lib):
    """x_{344+k} = sum_i W[i][k] r_i (mod 2^32): emulate the device GlibcWave in numpy."""
    class T(C.Structure):
        _fields_ = [("pow_even", C.c_uint32 * 64), ("pow128", C.c_uint32), ("pow512", C.c_uint32), ("inv16807", C.c_uint32), ("pow_lcg", C.c_uint32 * 31),
                    ("w_init", C.c_uint32 * (31 * 64)), ("w_next", C.c_uint32 * (31 * 64)), ("pad", C.c_uint32 * 2)]
    t = T()
    assert gpu_lib._f("dbg_tables")(C.byref(t), C.sizeof(t)) == 0
    M = 2147483647
    assert [int(x) for x in t.pow_even][:3] == [pow(16807, 2, M), pow(16807, 4, M), pow(16807, 6, M)]
    assert (int(t.inv16807) * 16807) % M == 1
    assert int(t.pow128) == pow(16807, 128, M) and int(t.pow512) == pow(16807, 512, M)
    w_init = np.array(t.w_init, dtype=np.uint64).reshape(31, 64)
    w_next = np.array(t.w_next, dtype=np.uint64).reshape(31, 64)
    for seed in [0, 1, 12345, 2147483646, 2147483647, 2147483648, 4294967295, 987654321]:
        s = seed if seed else 1
        w0 = s - (1 << 32) if s >= (1 << 31) else s
        hi, lo = int(w0 / 127773), int(np.fmod(w0, 127773))          # C truncating division
        w = 16807 * lo - 2836 * hi
        if w < 0:
            w += M
        r = np.zeros(31, dtype=np.uint64)
        r[0] = s
        for i in range(1, 31):
            r[i] = (pow(16807, i - 1, M) * w) % M
        assert int(t.pow_lcg[5]) == pow(16807, 4, M)
        x = (r[:, None] * w_init).sum(axis=0) & 0xFFFFFFFF                  # block 0
        out = list(x >> 1)
        for _ in range(2):                                                  # two more blocks
            x = (x[33:64, None] * w_next).sum(axis=0) & 0xFFFFFFFF
            out += list(x >> 1)
        want = oracle_api.kat_rand(oracle_lib, seed, 192)
        assert [int(v) for v in out] == [int(v) for v in want], f"seed {seed}"


def test_cpp_host_fails_loudly_without_gpu():
    """error convention of the reference's seam: message on stdout, failure status, no exception across the ABI"""
    import subprocess
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    exe = os.path.join(ROOT, "tools", "host_demo")
    if not os.path.exists(exe):
        pytest.skip("tools/host_demo not built (run __graft_entry__.build())")
    r = subprocess.run([exe, "10", "100", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stdout
