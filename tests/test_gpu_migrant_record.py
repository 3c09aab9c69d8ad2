"""The packed migrant record of gev_export_rows / gev_import_rows, decoded in numpy (tests/helpers.py: decode_record, written from the
format comment of geneevolve_amd/csrc/gev_migrant_record.h, not from its code) and compared section by section with what the library's download calls
say about the exported individuals (pytest -m gpu)."""
import numpy as np
import pytest

from geneevolve_amd.capi import unpack_rows
from geneevolve_amd.host import Simulation
from tests import helpers

pytestmark = pytest.mark.gpu

SIZES, LS, N_CV, WHO = [12, 9], [130, 64], [5, 3], [7, 0, 11]


def scenario(gpu_lib, rows, track):
    """one context: populations of 12 and 9, chromosomes of 130 and 64 loci, two phenotypes of 5 and 3 CVs per chromosome, dense
    state, hot mutation map, two generations (the lists live as pieces) -> (context, Simulation, SNP positions, CV positions)"""
    nchr, rs = len(LS), np.random.RandomState(2718)
    g = gpu_lib.create(2, nchr, 2)
    g.set_dense_state(True); g.set_track_intervals(track); g.set_migrant_rows(rows)
    R, step = 61, 1000
    bp = (500 + step * np.arange(R)).astype(np.uint64)
    prob, rate = np.r_[0.0, np.full(R - 1, 0.02)], np.r_[0.0, np.full(R - 1, 0.1)]       # ~6 new mutations per gamete and generation
    snp_pos, cv_pos = [], [[], []]
    for c in range(nchr):
        pos = np.sort(rs.choice(np.arange(600, 60000), LS[c], replace=False)).astype(np.uint64)
        snp_pos.append(pos)
        for p in range(2):
            g.set_rmap(p, c, bp, prob, step); g.set_mutmap(p, c, bp, rate); g.set_snps(p, c, pos)
        for ph in range(2):
            cvbp = rs.choice(np.arange(600, 60000, 7), N_CV[ph], replace=False).astype(np.uint64)     # not in position order
            cv_pos[ph].append(cvbp)
            a, d = rs.randn(N_CV[ph]), rs.randn(N_CV[ph])
            for p in range(2):
                g.set_cvs(p, ph, c, cvbp, a, d, 0.0)
        for p in range(2):
            g.synth_founders(p, c, 2 * SIZES[p], 100 + 10 * p + c); g.synth_founder_panel(p, c, 2 * SIZES[p], 100 + 10 * p + c)
            for ph in range(2):
                g.synth_cv_founders(p, ph, c, 2 * SIZES[p], 200 + 10 * p + c + 100 * ph)
    sim = Simulation(g, 91, nchr, True)
    for p in range(2):
        sim.ras_initial_human_gen0(p, SIZES[p])
    for _ in range(2):
        for p in range(2):
            sim.next_generation_rm(p, SIZES[p])
    return g, sim, snp_pos, cv_pos


def export_record(g, pop, who):
    """the record of `who`, exported into a zero-filled device buffer of export_size bytes -> (bytes, device pointer, free())"""
    nb = g.export_size(pop, who)
    dev, free = helpers.device_buffer(nb, zero=True)
    g.export_rows(pop, who, dev, nb)
    return helpers.read_device_u32(dev, nb // 4).view(np.uint8), dev, free


def _lists_of(off, data, rows):
    return [data[int(off[r]):int(off[r + 1])] for r in rows]


@pytest.mark.parametrize("rows,track", [(True, True), (True, False), (False, True), (False, False)])
def test_record_sections_equal_the_downloads_and_import_restores_them(gpu_lib, rows, track):
    """Individuals 7, 0, 11 of population 0 (not in order) as a record: its size, counts, sexes, genotype rows (pool rows: compared
    where the row's own mutation list names no locus), CV rows, mutation and interval lists equal what the download calls give for
    them; imported into population 1 (refused without rows and intervals, so not tried then) the three new individuals' rows, CV rows
    and lists equal population 0's."""
    g, sim, snp_pos, cv_pos = scenario(gpu_lib, rows, track)
    nchr, n = len(LS), len(WHO)
    hrows = [2 * i + h for i in WHO for h in range(2)]
    rec, dev, free = export_record(g, 0, WHO)
    d = helpers.decode_record(rec, n, LS, cv_pos, 2, rows)
    assert d["total"] == len(rec) == g.export_size(0, WHO)
    assert np.array_equal(d["sex"], sim.sex[0][WHO]), "sexes"
    haps, cvs, muts, parts = [], [], [], []
    for k in range(nchr):
        m, moff = g.download_mutations(0, k)
        muts.append(_lists_of(moff, m, hrows))
        assert np.array_equal(d["counts"][:, k, :, 0].ravel(), [len(x) for x in muts[k]]), f"mutation counts chr {k}"
        assert np.array_equal(d["muts"][k], np.concatenate(muts[k])), f"mutation lists chr {k}"
        assert sum(len(x) for x in muts[k]) > 0, "the scenario was meant to have mutations"
        if track:
            q, qoff = g.download_intervals(0, k)
            parts.append(_lists_of(qoff, q, hrows))
            assert np.array_equal(d["counts"][:, k, :, 1].ravel(), [len(x) for x in parts[k]]), f"interval counts chr {k}"
            assert np.array_equal(d["parts"][k], np.concatenate(parts[k])), f"interval lists chr {k}"
        else:
            assert not d["counts"][:, k, :, 1].any() and len(d["parts"][k]) == 0, f"interval lists without interval tracking chr {k}"
        haps.append(unpack_rows(g.download_haps(0, k), LS[k])[hrows])
        if rows:
            for j, r in enumerate(hrows):
                named = np.isin(snp_pos[k], muts[k][j])
                assert named.sum() <= len(muts[k][j]) and 2 * (~named).sum() >= LS[k], f"loci compared in row {r} chr {k}"
                assert np.array_equal(d["rows"][k][j][~named], haps[k][j][~named]), f"genotype row {r} chr {k}"
        else:
            assert d["rows"][k] is None
        cvs.append([unpack_rows(g.download_cv(0, ph, k), N_CV[ph])[hrows] for ph in range(2)])
        for ph in range(2):
            assert np.array_equal(d["cv"][ph][k], cvs[k][ph]), f"CV rows phenotype {ph} chr {k}"
    if rows or track:
        g.import_rows(1, dev, len(rec), n)
        assert g.pop_size(1) == SIZES[1] + n
        new = list(range(2 * SIZES[1], 2 * (SIZES[1] + n)))
        for k in range(nchr):
            assert np.array_equal(unpack_rows(g.download_haps(1, k), LS[k])[new], haps[k]), f"imported genotype rows chr {k}"
            for ph in range(2):
                assert np.array_equal(unpack_rows(g.download_cv(1, ph, k), N_CV[ph])[new], cvs[k][ph]), f"imported CV rows phenotype {ph} chr {k}"
            m, moff = g.download_mutations(1, k)
            assert all(np.array_equal(x, y) for x, y in zip(_lists_of(moff, m, new), muts[k])), f"imported mutation lists chr {k}"
            if track:
                q, qoff = g.download_intervals(1, k)
                assert all(np.array_equal(x, y) for x, y in zip(_lists_of(qoff, q, new), parts[k])), f"imported interval lists chr {k}"
    free()
    g.close()


def test_record_of_nobody(gpu_lib):
    """export_size of zero individuals is the decoder's total for n = 0"""
    g, _, _, cv_pos = scenario(gpu_lib, True, True)
    assert g.export_size(0, []) == helpers.decode_record(np.zeros(0, dtype=np.uint8), 0, LS, cv_pos, 2, True)["total"]
    g.close()
