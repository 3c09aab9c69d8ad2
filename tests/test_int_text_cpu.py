"""The .int interval file's line formatter (geneevolve_amd/csrc/gev_fmt_int.h) compiled for the host, gev_dbg_format_interval_text_host:
every .int file the fixtures record reproduced byte for byte from the recorded lists, the integer edges of every numeric column against
Python's own str(), slices, the size query, short buffers and a name table that is too short."""
import numpy as np
import pytest

from geneevolve_amd import capi
from tests import helpers
from tests import int_text_inputs as T


def test_every_recorded_int_file_byte_for_byte(gpu_lib):
    """the reference's own SHA-256 of each .int file against the host build on the recorded ids and interval lists"""
    compared = lines = 0
    for name in T.FIXTURES:
        fx = helpers.load_fixture(name)
        names = T.founder_names(fx)
        for key, g, ip, ic, pre, label in T.recorded_files(fx):
            parts, off, ids = T.parts_of(fx[f"{pre}chr{ic}_parts"]), fx[f"{pre}chr{ic}_part_off"], fx[pre + "ids"][:, 0]
            txt = gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names)
            assert np.array_equal(T.sha256(txt), fx[key]), f"{name}: {key} differs from the reference's file"
            assert txt.count(b"\n") == len(parts) + 1
            compared += 1; lines += len(parts)
    print(f"{compared} files, {lines} lines")
    assert compared == T.N_RECORDED_FILES
    assert lines == 124644
    ex = helpers.load_fixture("ex1full")                      # left out: no parts recorded at its last generation
    assert all(f"{pre}chr{ic}_parts" not in ex for _, _, _, ic, pre, _ in T.recorded_files(ex))


EDGES = sorted({0, 9, 10, 2**32 - 1, 2**32, 2**63 - 1, 2**64 - 1} | {10**k - 1 for k in range(1, 20)} | {10**k for k in range(1, 20)})


def edge_case():
    """one individual per edge value: ID + 1, st and en each run through every value; hap_index + 1 through every edge its name table
    allows (0 .. 100002, even and odd); root_population + 1 through one and two digits; names of 1 to 64 bytes"""
    rng = np.random.default_rng(5)
    n = len(EDGES)
    n_names = [50001] + [3] * 11
    names = [["y" * 64 if k == 0 else "x" if k % 4 == 0 else "n" * (1 + (k * 7 + p) % 64) for k in range(m)] for p, m in enumerate(n_names)]
    haps = [0, 1, 8, 9, 98, 99, 998, 999, 9998, 9999, 99998, 99999, 100000, 100001]
    ids = np.array([(v - 1) % 2**64 for v in EDGES], dtype=np.uint64).view(np.int64)
    assert ids[0] == -1                                        # ID = -1 prints 0
    rows, off = [], [0]
    for i in range(n):
        for ihap in range(2):
            for j in range(1 + (i + ihap) % 3):
                rp = 0 if (i + j) % 2 == 0 else 1 + (i + j + ihap) % 11
                h = haps[(i + 3 * j + ihap) % len(haps)] if rp == 0 else int(rng.integers(0, 6))
                rows.append((EDGES[i] if j == 0 else EDGES[int(rng.integers(n))], EDGES[n - 1 - i] if j == 0 else EDGES[int(rng.integers(n))], h, rp))
            off.append(len(rows))
    parts = np.zeros(len(rows), dtype=capi.PART_DTYPE)
    for q, (st, en, h, rp) in enumerate(rows):
        parts[q] = (st, en, h, rp, 0)
    assert set(parts["st"].tolist()) >= set(EDGES) and set(parts["en"].tolist()) >= set(EDGES)
    assert set(parts["hap_index"][parts["root_population"] == 0].tolist()) == set(haps)
    assert {9, 10, 11} <= set(parts["root_population"].tolist())
    return parts, np.array(off, dtype=np.uint64), ids, names


@pytest.mark.parametrize("label", [7, 22, 123])
def test_integer_edges_in_every_column(gpu_lib, label):
    parts, off, ids, names = edge_case()
    got = gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names)
    want = T.py_text(parts, off, ids, label, names)
    if got != want:
        la, lb = got.split(b"\n"), want.split(b"\n")
        first = next(i for i, (a, b) in enumerate(zip(la, lb)) if a != b)
        raise AssertionError(f"line {first}: {la[first]!r} vs {lb[first]!r}")
    longest = max(len(x) for x in want.split(b"\n")) + 1
    assert longest <= 177 and b" " + b"y" * 64 + b".1 " in want and b" x.2 " in want
    assert b"\n0 %d 0 0 " % label in want                      # ID = -1, st = 0


def test_slices_size_query_and_refusals(gpu_lib):
    fx = helpers.load_fixture("mig3c")
    names = T.founder_names(fx)
    key, g, ip, ic, pre, label = T.recorded_files(fx)[0]
    parts, off, ids = T.parts_of(fx[f"{pre}chr{ic}_parts"]), fx[f"{pre}chr{ic}_part_off"], fx[pre + "ids"][:, 0]
    n = len(ids)
    whole = gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names)
    assert whole == T.py_text(parts, off, ids, label, names) and np.array_equal(T.sha256(whole), fx[key])
    rng = np.random.default_rng(11)
    for _ in range(4):
        cuts = [0] + sorted(int(x) for x in rng.integers(0, n + 1, size=5)) + [n]          # arbitrary boundaries, empty slices among them
        pieces = [gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names, header=(j == 0), ind_begin=a, n_ind=b - a) for j, (a, b) in enumerate(zip(cuts, cuts[1:]))]
        assert b"".join(pieces) == whole, f"slices at {cuts}"
    assert gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names, n_ind=0) == T.HEADER
    assert gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names, n_ind=0, header=False) == b""
    assert gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names, ind_begin=n, n_ind=0, header=False) == b""
    # a buffer of exactly the size, one byte too few (GEV_EINVAL, the size needed reported), far too many
    assert gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names, out_bytes=len(whole)) == whole
    assert gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names, out_bytes=len(whole) + 1000) == whole
    with pytest.raises(capi.GevError) as e:
        gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names, out_bytes=len(whole) - 1)
    assert e.value.code == -1 and "needed" in str(e.value) and gpu_lib.last_bytes_written == len(whole)
    # a name table that is too short: the largest founder index in use has no name
    rp = int(parts["root_population"][np.argmax(parts["hap_index"])])
    short = [list(x) for x in names]
    short[rp] = short[rp][:int(parts["hap_index"].max()) // 2]
    with pytest.raises(capi.GevError) as e:
        gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, short)
    assert e.value.code == -1 and "beyond" in str(e.value)
    with pytest.raises(capi.GevError) as e:                    # and a root population without a table
        gpu_lib.dbg_format_interval_text_host(parts, off, ids, label, names[:1])
    assert e.value.code == -1 and "no names" in str(e.value)
