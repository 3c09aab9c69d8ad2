"""Inputs and the C library's own answers for the %g tests (tests/test_info_text_cpu.py, tests/test_gpu_info_text.py)."""
import ctypes as C
import functools
import struct
from fractions import Fraction

import numpy as np

_libc = C.CDLL(None)
_libc.snprintf.restype = C.c_int

DBL_MIN, DBL_MAX = 2.2250738585072014e-308, 1.7976931348623157e308
NAN_POS = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
NAN_NEG = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]

EDGES = [0.0, -0.0, 1.0, 0.1, 100000.0, 999999.0, 999999.5, 999999.4999999999, 1e6, 1000005.0, 1000015.0, 100000.5, 100001.5, 10000.25, 10000.75,
         1000.125, 1000.375, 1e-4, 1e-5, 9.999995e-05, 9.9999949999e-05, 5e-324, DBL_MIN, DBL_MAX, float("inf"), float("-inf"), NAN_POS, NAN_NEG,
         1e22, 1e23, 1e100, 123456789.0]
# what the issue states for some of them, independent of any formatter
EDGES_STATED = {999999.5: b"1e+06", 1000005.0: b"1e+06", 1000015.0: b"1.00002e+06", 100000.5: b"100000", 100001.5: b"100002", 1e-5: b"1e-05",
                9.999995e-05: b"0.0001"}


def glibc_g(v):
    buf = C.create_string_buffer(64)
    _libc.snprintf(buf, C.c_size_t(64), b"%g", C.c_double(v))
    return buf.value


def expected(x):
    """%g of every value: Python's formatter for finite values (it agrees with glibc there), glibc for the rest"""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    return [(b"%g" % v) if f else glibc_g(v) for v, f in zip(x.tolist(), fin.tolist())]


@functools.lru_cache(maxsize=None)
def random_patterns(n=1 << 18):
    return np.random.default_rng(20240521).integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)


@functools.lru_cache(maxsize=None)
def near_midpoints(n=1 << 16):
    """for n random (d, k): the double nearest (d + 1/2) * 10^k and its two neighbours"""
    rs = np.random.default_rng(77)
    d = rs.integers(100000, 1000000, n); k = rs.integers(-328, 304, n)
    def nearest(fr):
        try:
            return float(fr)
        except OverflowError:                      # beyond DBL_MAX (k = 303 with d >= 179769)
            return float("inf")
    mid = np.array([nearest(Fraction(2 * int(a) + 1, 2) * Fraction(10) ** int(b)) for a, b in zip(d, k)])
    mid = mid[np.isfinite(mid) & (mid > 0)]        # (and the ones that round to zero below the subnormals)
    return np.concatenate([mid, np.nextafter(mid, 0.0), np.nextafter(mid, np.inf)])


@functools.lru_cache(maxsize=None)
def normals(n=1 << 18):
    return np.random.default_rng(5).standard_normal(n)


def strings(out16):
    return [bytes(r).rstrip(b"\0") for r in np.asarray(out16)]
