"""The hand-built migrant records of tests/migrant_inputs.py without a GPU: the encoder of the packed record (helpers.encode_record,
written from the format comment of geneevolve_amd/csrc/gev_migrant_record.h) against its decoder, and the oracle as the holder of the
truth model -- after gevo_import_rows of the same individuals its lists, genotype rows and CV rows equal the module's plain rasters,
which is what licenses those rasters as the reference of tests/test_gpu_migrant_import.py."""
import numpy as np
import pytest

from geneevolve_amd.capi import unpack_rows
from tests import helpers
from tests import migrant_inputs as M


@pytest.mark.parametrize("rows_travel", [True, False])
@pytest.mark.parametrize("active", [None, [True, False]])
@pytest.mark.parametrize("which", ["first", "second"])
def test_decode_of_encode_returns_the_individuals(rows_travel, active, which):
    """section by section; the total is the decoder's (tools/migrant_record_check.cpp, which pins migrant_record_layout's, is a
    stand-alone program and not reachable from here).  An inactive chromosome has zero counts and no bytes."""
    inds = M.IMMIGRANTS if which == "first" else M.IMMIGRANTS_B
    n = len(inds)
    rec, mask = M.encode(inds, rows_travel, active=active, want_mask=True)
    d = helpers.decode_record(rec, n, M.LS, M.CV_POS, M.N_POP, rows_travel, active=active)
    assert d["total"] == len(rec) == len(mask)
    assert not rec[~mask].any(), "padding bytes are zero"
    assert np.array_equal(d["sex"], [ind["sex"] for ind in inds])
    on = [True] * M.NCHR if active is None else active
    for k in range(M.NCHR):
        parts, poff, muts, moff = M.lists_as_downloaded(inds, k)
        if not on[k]:
            assert not d["counts"][:, k].any() and d["rows"][k] is None and len(d["muts"][k]) == 0 and len(d["parts"][k]) == 0
            assert all(d["cv"][p][k] is None for p in range(M.NPHEN))
            continue
        assert np.array_equal(d["counts"][:, k, :, 0].ravel(), np.diff(moff.astype(np.int64))), f"mutation counts chr {k}"
        assert np.array_equal(d["counts"][:, k, :, 1].ravel(), np.diff(poff.astype(np.int64))), f"part counts chr {k}"
        assert np.array_equal(d["muts"][k], muts) and d["parts"][k].tobytes() == parts.tobytes(), f"lists chr {k}"
        if rows_travel:
            assert np.array_equal(d["rows"][k], M.raster_rows(inds, k, mutations=False)), f"pool rows chr {k}"
        else:
            assert d["rows"][k] is None
        for p in range(M.NPHEN):
            assert np.array_equal(d["cv"][p][k], M.raster_cv(inds, p, k)), f"CV rows phenotype {p} chr {k}"


def test_root_population_planes_of_the_cv_rows():
    """behind the alleles of a CV row: one plane per bit of the root population of the part that covers the CV, columns by position"""
    inds = M.IMMIGRANTS
    n, rec = len(inds), M.encode(M.IMMIGRANTS, False)
    at = helpers._up(helpers.record_sex_offset(n, M.NCHR) + n, 16)
    seen = set()
    for p in range(M.NPHEN):
        for k in range(M.NCHR):
            C = M.N_CV[p][k]; sub = max(-(-C // 32), 1); words = helpers._up(3 * sub, 4)
            raw = rec[at:at + 2 * n * words * 4].view(np.uint32).reshape(2 * n, words); at += 2 * n * words * 4
            assert at % 16 == 0
            order = np.argsort(M.CV_POS[p][k], kind="stable")
            for r, (parts, _) in enumerate(M.rows_of(inds, k)):
                rp = np.array([M._covering_part(parts, int(x))[1] for x in M.CV_POS[p][k][order]])
                for b in range(2):
                    assert np.array_equal(unpack_rows(raw[r:r + 1, (1 + b) * sub:(2 + b) * sub], C)[0], (rp >> b) & 1), (p, k, r, b)
                    assert not unpack_rows(raw[r:r + 1, (1 + b) * sub:(2 + b) * sub], 32 * sub)[0][C:].any()
                seen.update(rp.tolist())
    assert seen == {0, 1, 2}


def test_the_encoder_refuses_lists_the_library_cannot_hold():
    good = M.IMMIGRANTS_B

    def changed(edit):
        inds = [{"sex": ind["sex"], "chr": [[(list(p), list(m)) for p, m in pair] for pair in ind["chr"]]} for ind in good]
        edit(inds[0]["chr"][0][0])
        return inds

    def gap(row): row[0][1] = (row[0][1][0] + 1,) + row[0][1][1:]
    def late(row): row[0][0] = (row[0][0][0] + 1,) + row[0][0][1:]
    def short(row): row[0][-1] = row[0][-1][:1] + (row[0][-1][1] - 1,) + row[0][-1][2:]
    def pop(row): row[0][2] = row[0][2][:3] + (M.N_POP,)
    def hap(row): row[0][2] = row[0][2][:2] + (M.n_founders(row[0][2][3]), row[0][2][3])
    def twice(row): row[1][1] = row[1][0]
    for edit in (gap, late, short, pop, hap, twice):
        with pytest.raises(AssertionError):
            M.encode(changed(edit), True)
    M.encode(changed(lambda row: None), True)
    with pytest.raises(AssertionError):                        # a mutation no part covers: the oracle cannot hold it
        helpers.encode_oracle_record(changed(lambda row: row[1].append(M.BP_END[0])))


@pytest.fixture(scope="module")
def oracle_with_immigrants(oracle_lib):
    """population 0 of the oracle at generation 0 with the first record imported, then the second"""
    o = oracle_lib.create(M.N_POP, M.NCHR, M.NPHEN)
    M.apply_static(o, device=False)
    for pop in range(M.N_POP):
        o.init_gen0(pop, M.RESIDENTS[pop], 300 + pop)
    words = []
    for inds in (M.IMMIGRANTS, M.IMMIGRANTS_B):
        w = helpers.encode_oracle_record(inds); words.append(w)
        o.import_rows(0, w.ctypes.data, w.nbytes, len(inds))
    yield o, words
    o.close()


def test_the_oracle_holds_the_truth_model(oracle_with_immigrants):
    """lists, genotype rows and CV rows of the imported rows equal the input and its rasters; the residents in front are untouched;
    export gives the imported words back"""
    o, words = oracle_with_immigrants
    n0 = M.RESIDENTS[0]
    everyone = M.IMMIGRANTS + M.IMMIGRANTS_B
    assert o.pop_size(0) == n0 + len(everyone)
    for k in range(M.NCHR):
        want_parts, want_poff, want_muts, want_moff = M.lists_as_downloaded(everyone, k)
        parts, poff = o.download_intervals(0, k); muts, moff = o.download_mutations(0, k)
        assert np.array_equal(poff[:2 * n0 + 1], np.arange(2 * n0 + 1)) and not moff[:2 * n0 + 1].any(), "the residents' lists"
        assert np.array_equal(poff[2 * n0:] - poff[2 * n0], want_poff) and parts[2 * n0:].tobytes() == want_parts.tobytes(), f"interval lists chr {k}"
        assert np.array_equal(moff[2 * n0:], want_moff) and np.array_equal(muts, want_muts), f"mutation lists chr {k}"
        haps = unpack_rows(o.download_haps(0, k), M.LS[k])
        assert np.array_equal(haps[:2 * n0], M.FOUNDERS[k][0]), f"the residents' rows chr {k}"
        assert np.array_equal(haps[2 * n0:], M.raster_rows(everyone, k)), f"genotype rows chr {k}"
        for p in range(M.NPHEN):
            cv = unpack_rows(o.download_cv(0, p, k), M.N_CV[p][k])
            assert np.array_equal(cv[:2 * n0], M.CV_FOUNDERS[p][k][0]) and np.array_equal(cv[2 * n0:], M.raster_cv(everyone, p, k)), f"CV rows phenotype {p} chr {k}"
    at = n0
    for inds, w in zip((M.IMMIGRANTS, M.IMMIGRANTS_B), words):
        who = np.arange(at, at + len(inds), dtype=np.uint64); at += len(inds)
        nb = o.export_size(0, who)
        back = np.zeros(nb // 8, dtype=np.uint64)
        o.export_rows(0, who, back.ctypes.data, nb)
        assert np.array_equal(back, w), "the oracle's export of the imported individuals"


def test_host_builds_of_the_list_readers_on_the_immigrants_lists(gpu_lib):
    """the arithmetic k_ibd_tiles / k_ibd_segments share with their host build, on the crafted rows themselves (the GPU file runs the
    kernels): equal to the position rasters, all pairs, the upper triangle and a min_bp in the middle of the tract lengths"""
    from tests import ibd_segments_inputs as S
    for k in range(M.NCHR):
        parts, poff, _, _ = M.lists_as_downloaded(M.IMMIGRANTS + M.IMMIGRANTS_B, k)
        runs = S.all_runs(parts, poff)
        lengths = sorted(en - st for row in runs for cell in row for st, en in cell)
        for min_bp in (0, lengths[len(lengths) // 3]):
            sh, ns, mx = gpu_lib.dbg_ibd_host(parts, poff, min_bp=min_bp)
            for a in range(len(runs)):
                for b in range(len(runs)):
                    s = [en - st for st, en in runs[a][b] if en - st >= min_bp]
                    assert (int(sh[a, b]), int(ns[a, b]), int(mx[a, b])) == (sum(s), len(s), max(s, default=0)), (k, min_bp, a, b)
            S.same(gpu_lib.dbg_ibd_segments_host(parts, poff, min_bp=min_bp), S.records(runs, min_bp=min_bp), f"segments chr {k} min_bp {min_bp}")
            S.same(gpu_lib.dbg_ibd_segments_host(parts, poff, min_bp=min_bp, upper=True), S.records(runs, min_bp=min_bp, upper=True), f"upper triangle chr {k} min_bp {min_bp}")
