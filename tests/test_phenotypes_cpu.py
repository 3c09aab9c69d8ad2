"""CPU specification of the parental-effect gather of ras_scale_AD_compute_GEF (reference src/Simulation.cpp:3118-3131) and the
ctypes surface of the device pedigree: host.parental_inputs against the reference's own recorded inputs, with the saved record
(_Pop_info_prev_gen, :3211-3236) rebuilt from the recorded outputs of the generation before and the recorded migration."""
import numpy as np
import pytest

from geneevolve_amd import capi
from geneevolve_amd.host import Pedigree, parental_inputs
from tests import helpers


def carried(fx, g, per_pop):
    """per-population arrays of generation g's individuals after generation g's migration: stayers keep their order
    (:960-966), migrants are appended in move order (:971-981)"""
    if f"g{g}_moves" not in fx:
        return [np.asarray(a) for a in per_pop]
    moves = helpers.derive_moves(fx, g)
    out = []
    for ip, a in enumerate(per_pop):
        gone = np.zeros(len(a), dtype=bool)
        for sp, pos, dp in moves:
            if sp == ip:
                gone[pos] = True
        parts = [np.asarray(a)[~gone]] + [np.asarray(per_pop[sp])[pos:pos + 1] for sp, pos, dp in moves if dp == ip]
        out.append(np.concatenate(parts))
    return out


def saved_record(fx, g, p, column):
    """_Pop_info_prev_gen of every population as generation g's phenotype step finds it: column 5 (phen) or 4 (parental_effect)
    of generation g-1's recorded outputs, carried through generation g-1's migration"""
    n_pop = int(fx["n_pop"])
    return carried(fx, g - 1, [fx[f"g{g - 1}_pop{ip}_ph{p}_gef_out"][:, column] for ip in range(n_pop)])


@pytest.mark.parametrize("case,pops", [("dense", [0]), ("vt2", [0]), ("mig3c", [0])])
def test_parental_inputs_reproduce_the_reference_recorded_inputs(case, pops):
    fx = helpers.load_fixture(case)
    nphen, ngen = int(fx["nphen"]), int(fx["n_gen"])
    n_checked = 0
    for g in range(2, ngen + 1):
        for p in range(nphen):
            vt = int(fx[f"g{g}_pop0_ph{p}_gef_vt"])
            prev = saved_record(fx, g, p, 5 if vt == 1 else 4)
            for ip in pops:
                ids = fx[f"g{g}_pop{ip}_ids"]
                assert int(ids[:, 1:3].max()) < len(prev[ip])
                got = parental_inputs(prev[ip], ids)
                assert helpers.bits_equal(got, fx[f"g{g}_pop{ip}_ph{p}_gef_in"][:, 1:3]), f"{case}: parental inputs, generation {g} population {ip} phenotype {p}"
                n_checked += 1
    assert n_checked >= ngen - 1


def test_parental_inputs_index_by_id_not_by_position():
    """mig3c population 0 after a migration: ids and positions differ, and the recorded inputs follow the ids"""
    fx = helpers.load_fixture("mig3c")
    differ = 0
    for g in range(2, int(fx["n_gen"]) + 1):
        post = fx[f"g{g - 1}_pop0_postmig_ids"]
        assert len(post) == len(saved_record(fx, g, 0, 5)[0])
        differ += int(np.sum(post[:, 0] != np.arange(len(post))))
    assert differ > 0


def test_parental_inputs_refuse_ids_beyond_the_saved_record():
    """mig3c population 1: the reference itself reads past the end of its saved array (ids up to 99, 86 saved entries)"""
    fx = helpers.load_fixture("mig3c")
    n_bad = {}
    for g in range(2, int(fx["n_gen"]) + 1):
        prev = saved_record(fx, g, 0, 5)[1]
        ids = fx[f"g{g}_pop1_ids"]
        bad = int(np.sum((ids[:, 1] >= len(prev)) | (ids[:, 2] >= len(prev))))
        n_bad[g] = (bad, len(ids), len(prev))
        if bad:
            with pytest.raises(IndexError):
                parental_inputs(prev, ids)
    assert n_bad[2] == (11, 90, 86) and n_bad[3] == (3, 90, 86) and n_bad[4] == (9, 90, 86), n_bad


def test_parental_inputs_accept_a_pedigree_and_check_negative_ids():
    prev = np.arange(10, dtype=np.float64) * 1.5
    P = Pedigree(4)
    P.ID_Father = np.array([9, 0, 3, 3]); P.ID_Mother = np.array([1, 1, 2, 8])
    assert np.array_equal(parental_inputs(prev, P), np.stack([prev[P.ID_Father], prev[P.ID_Mother]], axis=1))
    P.ID_Mother = np.array([1, 1, -1, 8])
    with pytest.raises(IndexError):
        parental_inputs(prev, P)
    with pytest.raises(IndexError):
        parental_inputs(prev[:9], np.array([[0, 9, 1]]))


def test_pedigree_entry_points_are_declared_and_exported(gpu_lib):
    for name in ("set_track_pedigree", "download_pedigree", "upload_pedigree"):
        assert name in capi.ABI_SYMBOLS and gpu_lib.exports(name)
        assert hasattr(capi.GevContext, name)
