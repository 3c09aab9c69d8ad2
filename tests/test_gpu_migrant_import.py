"""gev_import_rows fed records the library did not write (pytest -m gpu).  Every other import of the suite takes a record the library
itself exported a moment earlier, so an error shared by export and import passes, and only lists a small simulation produces reach
k_lp_import, k_parts_locus_range, k_rebuild_rows and the readers behind them.  Here the records are encoded in numpy from hand-built
individuals (tests/migrant_inputs.py, helpers.encode_record -- written from the format comment of csrc/gev_migrant_record.h): rows of
hundreds of parts, 45 parts in one position range between two empty ones, parts and zero-length parts on range edges and at the last map
position, mutation lists of hundreds of entries on range edges, part boundaries, SNPs and CVs, founders of three root populations.

(a) the encoder against the library's own export; (b) the import, in every transport, list state and range width; (c) three generations
bred from the immigrants against the oracle; (d) the device's list readers over them.  Every comparison is equality of integers or
bytes; the only bytes left out are the padding between sections (at most 15 per section, asserted by the encoder)."""
import numpy as np
import pytest

from geneevolve_amd.capi import pack_rows, unpack_rows
from geneevolve_amd.host import Simulation
from tests import helpers
from tests import ibd_segments_inputs as S
from tests import migrant_inputs as M
from tests.synth import synth_bits

pytestmark = pytest.mark.gpu

N0 = M.RESIDENTS[0]
N_IMM, N_IMM_B = len(M.IMMIGRANTS), len(M.IMMIGRANTS_B)
FOUNDER_SEEDS = [[M.founder_seed(p, k) for p in range(M.N_POP)] for k in range(M.NCHR)]


# ---- (a) the encoder against the library --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,track", [(True, True), (True, False), (False, True), (False, False)])
def test_encoder_reproduces_the_librarys_own_record(gpu_lib, rows, track):
    """the scenario of test_gpu_migrant_record.py: the record of individuals 7, 0, 11 encoded from what the download calls say about them
    (lists, sexes) and the scenario's founders equals the exported bytes outside the padding between sections.  Without interval
    tracking the downloads give no parts: the parts then come from the same scenario run with tracking (the random streams do not depend
    on it) and travel in neither record."""
    from tests import test_gpu_migrant_record as R
    g, sim, snp_pos, cv_pos = R.scenario(gpu_lib, rows, track)
    nchr = len(R.LS)
    rec, _, free = R.export_record(g, 0, R.WHO)
    free()
    src, src_sim = (g, sim) if track else R.scenario(gpu_lib, rows, True)[:2]
    assert np.array_equal(src_sim.sex[0], sim.sex[0])
    inds = M.individuals_from_downloads(sim.sex[0][R.WHO], [src.download_intervals(0, k) for k in range(nchr)], [g.download_mutations(0, k) for k in range(nchr)], R.WHO)
    founders = [[synth_bits(100 + 10 * p + k, 2 * R.SIZES[p], R.LS[k]) for p in range(2)] for k in range(nchr)]
    cv_founders = [[[synth_bits(200 + 10 * p + k + 100 * ph, 2 * R.SIZES[p], R.N_CV[ph]) for p in range(2)] for k in range(nchr)] for ph in range(2)]
    span = [(500, 500 + 1000 * 60)] * nchr
    mine, mask = helpers.encode_record(inds, R.LS, cv_pos, 2, rows, founders=founders, cv_founders=cv_founders, snp_pos=snp_pos, span=span,
                                       parts_travel=track, want_mask=True)
    assert len(mine) == len(rec), f"{len(mine)} bytes encoded, {len(rec)} exported"
    bad = np.flatnonzero((mine != rec) & mask)
    assert len(bad) == 0, f"{len(bad)} bytes differ, first at {bad[:5].tolist()}"
    if src is not g:
        src.close()
    g.close()


# ---- the contexts of (b), (c), (d) ------------------------------------------------------------------------------------------------------
def device_context(gpu_lib, transport):
    """copied: genotype rows travel; rebuilt: they are rebuilt from the founder panels; plane_less: no genotype planes at all"""
    g = gpu_lib.create(M.N_POP, M.NCHR, M.NPHEN)
    dense = transport != "plane_less"
    g.set_dense_state(dense); g.set_track_intervals(True); g.set_migrant_rows(transport == "copied")
    M.apply_static(g, device=True, founder_rows=dense, panels=transport == "rebuilt")
    return g, dense


def start(ctx, bred, seed=300):
    """generation 0 of all populations (the lists live in CSR form); bred: two generations of population 0 on top (they live as pieces)"""
    sim = Simulation(ctx, seed, M.NCHR, True)
    for pop in range(M.N_POP):
        sim.ras_initial_human_gen0(pop, M.RESIDENTS[pop])
    for _ in range(2 if bred else 0):
        sim.next_generation_rm(0, N0)
    return sim


def import_record(g, rec, n):
    dev, free = helpers.device_buffer(len(rec))
    helpers.write_device(dev, rec)
    try:
        g.import_rows(0, dev, len(rec), n)
    finally:
        free()


def export_bytes(g, who):
    nb = g.export_size(0, who)
    dev, free = helpers.device_buffer(nb, zero=True)
    g.export_rows(0, who, dev, nb)
    out = helpers.read_device_u32(dev, nb // 4).view(np.uint8)
    free()
    return out


def founder_tiles(k):
    return [pack_rows(M.FOUNDERS[k][rp]) for rp in range(M.N_POP)]


def genotype_rows(g, dense, k):
    words = g.download_haps(0, k) if dense else g.materialize_pops(0, k, founder_tiles(k))
    return unpack_rows(words, M.LS[k])


def state_of(g, dense, chrs):
    """everything the downloads say about population 0, as bytes per item"""
    out = {}
    for k in chrs:
        parts, poff = g.download_intervals(0, k); muts, moff = g.download_mutations(0, k)
        out[k] = {"parts": parts, "poff": poff, "muts": muts, "moff": moff, "rows": genotype_rows(g, dense, k),
                  "cv": [unpack_rows(g.download_cv(0, p, k), M.N_CV[p][k]) for p in range(M.NPHEN)]}
    return out


def check_rows_behind(after, row0, individuals, k, what):
    """the rows of `individuals` from haplotype row row0 on equal the input and its rasters"""
    a, n2 = after[k], 2 * len(individuals)
    parts, poff, muts, moff = M.lists_as_downloaded(individuals, k)
    p0, m0 = int(a["poff"][row0]), int(a["moff"][row0])
    assert np.array_equal(a["poff"][row0:row0 + n2 + 1].astype(np.int64) - p0, poff.astype(np.int64)), f"{what}: interval offsets chr {k}"
    assert a["parts"][p0:p0 + len(parts)].tobytes() == parts.tobytes(), f"{what}: interval lists chr {k}"
    assert np.array_equal(a["moff"][row0:row0 + n2 + 1].astype(np.int64) - m0, moff.astype(np.int64)), f"{what}: mutation offsets chr {k}"
    assert np.array_equal(a["muts"][m0:m0 + len(muts)], muts), f"{what}: mutation lists chr {k}"
    want = M.raster_rows(individuals, k)
    bad = np.argwhere(a["rows"][row0:row0 + n2] != want)
    assert len(bad) == 0, f"{what}: genotype rows chr {k}: {len(bad)} bits differ, first (row, SNP) {bad[:4].tolist()}"
    for p in range(M.NPHEN):
        bad = np.argwhere(a["cv"][p][row0:row0 + n2] != M.raster_cv(individuals, p, k))
        assert len(bad) == 0, f"{what}: CV rows phenotype {p} chr {k}: first (row, CV) {bad[:4].tolist()}"


def check_residents(before, after, k, what):
    b, a, r = before[k], after[k], 2 * N0
    assert np.array_equal(a["poff"][:r + 1], b["poff"]) and a["parts"][:len(b["parts"])].tobytes() == b["parts"].tobytes(), f"{what}: the residents' interval lists chr {k}"
    assert np.array_equal(a["moff"][:r + 1], b["moff"]) and np.array_equal(a["muts"][:len(b["muts"])], b["muts"]), f"{what}: the residents' mutation lists chr {k}"
    assert np.array_equal(a["rows"][:r], b["rows"]), f"{what}: the residents' genotype rows chr {k}"
    for p in range(M.NPHEN):
        assert np.array_equal(a["cv"][p][:r], b["cv"][p]), f"{what}: the residents' CV rows phenotype {p} chr {k}"


def import_and_check(g, dense, transport, chrs, active=None):
    rows_travel = transport == "copied"
    before = state_of(g, dense, chrs)
    rec, mask = M.encode(M.IMMIGRANTS, rows_travel, active=active, want_mask=True)
    import_record(g, rec, N_IMM)
    assert g.pop_size(0) == N0 + N_IMM
    after = state_of(g, dense, chrs)
    for k in chrs:
        check_residents(before, after, k, "first import")
        check_rows_behind(after, 2 * N0, M.IMMIGRANTS, k, "first import")
        if dense:
            assert g.dbg_verify_planes(0, k, FOUNDER_SEEDS[k]) == (0, 0), f"planes != materialised intervals chr {k}"
    rec_b, mask_b = M.encode(M.IMMIGRANTS_B, rows_travel, active=active, want_mask=True)
    import_record(g, rec_b, N_IMM_B)
    assert g.pop_size(0) == N0 + N_IMM + N_IMM_B
    last = state_of(g, dense, chrs)
    for k in chrs:
        check_residents(before, last, k, "second import")
        check_rows_behind(last, 2 * N0, M.IMMIGRANTS, k, "the first record behind the second import")
        check_rows_behind(last, 2 * (N0 + N_IMM), M.IMMIGRANTS_B, k, "second import")
        if dense:
            assert g.dbg_verify_planes(0, k, FOUNDER_SEEDS[k]) == (0, 0), f"planes != materialised intervals chr {k} (second import)"
    for who, r, m, what in ((np.arange(N0, N0 + N_IMM), rec, mask, "first"), (np.arange(N0 + N_IMM, N0 + N_IMM + N_IMM_B), rec_b, mask_b, "second")):
        back = export_bytes(g, who.astype(np.uint64))
        assert len(back) == len(r), f"export of the {what} record: {len(back)} bytes, {len(r)} went in"
        bad = np.flatnonzero((back != r) & m)
        assert len(bad) == 0, f"export of the {what} record: {len(bad)} bytes differ from what went in, first at {bad[:5].tolist()}"


# ---- (b) the import ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_ranges", [32, 5])
@pytest.mark.parametrize("bred", [False, True], ids=["csr", "pieces"])
@pytest.mark.parametrize("transport", ["copied", "rebuilt", "plane_less"])
def test_import_of_the_hand_built_record(gpu_lib, monkeypatch, transport, bred, max_ranges):
    """on the new rows the downloads equal the input and its rasters, the planes equal the materialised intervals, the residents are
    unchanged bit for bit, a second record appends behind the first, and the export of the imported individuals returns the bytes that
    went in"""
    monkeypatch.setenv("GEV_LIST_SEGS", str(max_ranges))
    g, dense = device_context(gpu_lib, transport)
    start(g, bred)
    import_and_check(g, dense, transport, range(M.NCHR))
    g.close()


@pytest.mark.parametrize("transport", ["copied", "rebuilt"])
def test_import_with_chromosome_1_inactive(gpu_lib, transport):
    """a locus-split context: the record has zero counts and no bytes for chromosome 1"""
    g = gpu_lib.create(M.N_POP, M.NCHR, M.NPHEN)
    g.set_dense_state(True); g.set_track_intervals(True); g.set_migrant_rows(transport == "copied")
    g.set_chr_active(1, False)
    for pop in range(M.N_POP):
        for k in range(M.NCHR):
            g.set_rmap(pop, k, M.RMAP_BP[k], M.RMAP_PROB[k], M.MAP_STEP[k]); g.set_mutmap(pop, k, M.RMAP_BP[k], M.MUT_RATE[k])
        g.set_snps(pop, 0, M.SNP_POS[0])
        words = pack_rows(M.FOUNDERS[0][pop])
        g.upload_founders(pop, 0, words, M.LS[0])
        if transport == "rebuilt":
            g.upload_founder_panel(pop, 0, words, M.LS[0])
        for p in range(M.NPHEN):
            g.set_cvs(pop, p, 0, M.CV_POS[p][0], M.CV_A[pop][p][0], M.CV_D[pop][p][0], M.CV_VD)
            g.upload_cv_founders(pop, p, 0, pack_rows(M.CV_FOUNDERS[p][0][pop]), M.N_CV[p][0])
    start(g, True)
    rec = M.encode(M.IMMIGRANTS, transport == "copied", active=[True, False])
    assert not helpers.decode_record(rec, N_IMM, M.LS, M.CV_POS, M.N_POP, transport == "copied", active=[True, False])["counts"][:, 1].any()
    import_and_check(g, True, transport, [0], active=[True, False])
    g.close()


# ---- (c) breeding from them, against the oracle -------------------------------------------------------------------------------------------
def couples_of(sex, rs, first):
    """[male, female, 0, offspring]; first generation: every immigrant is a parent in two couples or more, one of them with another
    immigrant; later generations: a spread over everybody"""
    males, females = np.flatnonzero(sex == 1), np.flatnonzero(sex == 2)
    assert len(males) and len(females)
    out = []
    if first:
        imm = np.arange(N0, N0 + N_IMM)
        im, jf = [i for i in imm if sex[i] == 1], [i for i in imm if sex[i] == 2]
        assert len(im) == len(jf) == N_IMM // 2
        res_m, res_f = [i for i in males if i < N0], [i for i in females if i < N0]
        for q in range(len(im)):
            out.append((im[q], jf[q], 2)); out.append((im[q], jf[(q + 1) % len(jf)], 1))         # an immigrant with an immigrant
            out.append((im[q], res_f[q % len(res_f)], 1)); out.append((res_m[q % len(res_m)], jf[q], 1))
        out.append((res_m[-1], res_f[-1], 2))
        used = np.bincount([x for c in out for x in c[:2]], minlength=len(sex))
        assert (used[N0:N0 + N_IMM] >= 2).all()
    else:
        for q in range(len(sex)):
            out.append((males[(5 * q + 1) % len(males)], females[(3 * q + 2) % len(females)], 1 + (q % 7 == 0)))
    return np.array([(m, f, 0, k) for m, f, k in out], dtype=np.int64)


@pytest.mark.parametrize("transport,literal", [("copied", 0), ("copied", 1), ("rebuilt", 0), ("plane_less", 0)])
def test_breeding_from_the_immigrants_equals_the_oracle(gpu_lib, oracle_lib, monkeypatch, transport, literal):
    """three generations on a map that is hot around the crowded range: sexes, genotype rows, lists, CV rows, CV frequencies and A/D equal
    the oracle's bit for bit, every generation (lp_build_parts / lp_build_muts over imported pieces, k_cv_newmut's lookup in them)"""
    monkeypatch.setenv("GEV_LP_LITERAL", str(literal))
    g, dense = device_context(gpu_lib, transport)
    o = oracle_lib.create(M.N_POP, M.NCHR, M.NPHEN)
    M.apply_static(o, device=False)
    for pop in range(M.N_POP):
        sex0 = g.init_gen0(pop, M.RESIDENTS[pop], 300 + pop)
        assert np.array_equal(sex0, o.init_gen0(pop, M.RESIDENTS[pop], 300 + pop))
        if pop == 0:
            sex = np.r_[sex0, [ind["sex"] for ind in M.IMMIGRANTS]].astype(np.uint8)
    import_record(g, M.encode(M.IMMIGRANTS, transport == "copied"), N_IMM)
    w = helpers.encode_oracle_record(M.IMMIGRANTS)
    o.import_rows(0, w.ctypes.data, w.nbytes, N_IMM)
    who = np.arange(N0 + N_IMM, dtype=np.uint64)                       # the sexes the library holds now: the [sex] bytes of everybody's record
    assert np.array_equal(export_bytes(g, who)[helpers.record_sex_offset(len(who), M.NCHR):][:len(who)], sex)
    rs = np.random.RandomState(5)
    n_new_muts = 0
    for gen in (1, 2, 3):
        couples = couples_of(sex, rs, gen == 1)
        n = int(couples[:, 3].sum())
        seed, ms = int(rs.randint(1, 2 ** 31 - 1)), rs.randint(1, 2 ** 31 - 1, n * M.NCHR).astype(np.uint32)
        sex = g.reproduce(0, couples, seed, ms)
        assert np.array_equal(sex, o.reproduce(0, couples, seed, ms)), f"sexes, generation {gen}"
        for x, y, name in zip(g.compute_ad(0), o.compute_ad(0), ("additive", "dominance", "additive_chr", "dominance_chr")):
            assert helpers.bits_equal(x, y), f"{name}, generation {gen}"
        for k in range(M.NCHR):
            pg, og = g.download_intervals(0, k); po, oo = o.download_intervals(0, k)
            assert np.array_equal(og, oo) and pg.tobytes() == po.tobytes(), f"interval lists chr {k}, generation {gen}"
            mg, mog = g.download_mutations(0, k); mo, moo = o.download_mutations(0, k)
            assert np.array_equal(mog, moo) and np.array_equal(mg, mo), f"mutation lists chr {k}, generation {gen}"
            n_new_muts += len(mg)
            assert np.array_equal(genotype_rows(g, dense, k), unpack_rows(o.download_haps(0, k), M.LS[k])), f"genotype rows chr {k}, generation {gen}"
            for p in range(M.NPHEN):
                assert np.array_equal(g.download_cv(0, p, k), o.download_cv(0, p, k)), f"CV rows phenotype {p} chr {k}, generation {gen}"
                assert helpers.bits_equal(g.get_cv_freq(0, p, k), o.get_cv_freq(0, p, k)), f"CV frequencies phenotype {p} chr {k}, generation {gen}"
            if dense:
                assert g.dbg_verify_planes(0, k, FOUNDER_SEEDS[k]) == (0, 0), f"planes != materialised intervals chr {k}, generation {gen}"
        if gen == 1:                                                # the hot map cut inside the crowded range
            parts, off = g.download_intervals(0, 0)
            in_crowded = [int(((parts["st"][int(off[r]):int(off[r + 1])] >= M.edge(M.CROWDED)) & (parts["st"][int(off[r]):int(off[r + 1])] < M.edge(M.CROWDED + 1))).sum()) for r in range(len(off) - 1)]
            assert any(15 <= c < 45 for c in in_crowded), "a child was meant to inherit a cut piece of the crowded range"
    assert n_new_muts > 0
    g.close(); o.close()


# ---- (d) the list readers on the device ------------------------------------------------------------------------------------------------
def sharing_from_runs(run_lists, min_bp=0):
    """(shared_bp, n_seg, max_seg) [n_a][n_b] from [n_a][n_b] lists of (st, en)"""
    n_a, n_b = len(run_lists), len(run_lists[0])
    sh = np.zeros((n_a, n_b), dtype=np.uint64); ns = np.zeros((n_a, n_b), dtype=np.uint32); mx = np.zeros((n_a, n_b), dtype=np.uint64)
    for a in range(n_a):
        for b in range(n_b):
            s = [en - st for st, en in run_lists[a][b] if en - st >= min_bp]
            sh[a, b], ns[a, b], mx[a, b] = sum(s), len(s), max(s, default=0)
    return sh, ns, mx


def slice_lists(parts, off, r0, n):
    """the lists of rows [r0, r0 + n) as (parts, offsets) of their own"""
    a, b = int(off[r0]), int(off[r0 + n])
    return parts[a:b], (off[r0:r0 + n + 1] - off[r0]).astype(np.uint64)


@pytest.mark.parametrize("chunk", [0, 5])
@pytest.mark.parametrize("bred", [False, True], ids=["csr", "pieces"])
def test_list_readers_over_the_immigrants(gpu_lib, chunk, bred):
    """ibd_sharing, ibd_segments and ancestry_bp against the position rasters of the downloaded lists, the .int text against the host
    build, genotype counts and trait sums over the immigrants against numpy on raster_rows"""
    g, _ = device_context(gpu_lib, "copied")
    for pop in range(M.N_POP):
        g.set_founder_names(pop, [f"p{pop}f{i}" + "x" * (i % 9) for i in range(M.RESIDENTS[pop])])
    names = [[f"p{pop}f{i}" + "x" * (i % 9) for i in range(M.RESIDENTS[pop])] for pop in range(M.N_POP)]
    start(g, bred)
    import_record(g, M.encode(M.IMMIGRANTS, True), N_IMM)
    n = N0 + N_IMM
    g.dbg_output_chunk(chunk)
    r0, r_imm = 2 * (N0 - 3), 2 * N0                                 # three residents and the immigrants: 18 haplotype rows
    rs = np.random.RandomState(9)
    for k in range(M.NCHR):
        parts, off = g.download_intervals(0, k)
        assert parts[int(off[r_imm]):].tobytes() == M.lists_as_downloaded(M.IMMIGRANTS, k)[0].tobytes(), f"the immigrants' lists chr {k}"
        sp, so = slice_lists(parts, off, r0, 2 * n - r0)
        runs = S.all_runs(sp, so)
        nr = len(runs)
        # square
        for got, want, name in zip(g.ibd_sharing(k, 0, r0, nr, 0, r0, nr), sharing_from_runs(runs), ("shared_bp", "n_seg", "max_seg")):
            assert np.array_equal(got, want), f"ibd_sharing {name}, square, chr {k}"
        S.same(g.ibd_segments(k, 0, r0, nr, 0, r0, nr), S.records(runs, row_a0=r0, row_b0=r0), f"ibd_segments, square, chr {k}")
        S.same(g.ibd_segments(k, 0, r0, nr, 0, r0, nr, upper=True), S.records(runs, upper=True, row_a0=r0, row_b0=r0), f"ibd_segments, upper, chr {k}")
        # residents x immigrants, and a min_bp that removes some of the short tracts but not all
        na, nb = r_imm - r0, 2 * n - r_imm
        rect = [row[na:] for row in runs[:na]]
        lengths = sorted(en - st for row in rect for cell in row for st, en in cell)
        assert len(lengths) >= 4 and lengths[0] < lengths[-1], f"residents and immigrants were meant to share tracts (chr {k})"
        min_bp = lengths[len(lengths) // 2]
        if lengths[0] == min_bp:
            min_bp = next(x for x in lengths if x > lengths[0])
        assert 0 < sum(x >= min_bp for x in lengths) < len(lengths)
        for m in (0, min_bp):
            for got, want, name in zip(g.ibd_sharing(k, 0, r0, na, 0, r_imm, nb, min_bp=m), sharing_from_runs(rect, m), ("shared_bp", "n_seg", "max_seg")):
                assert np.array_equal(got, want), f"ibd_sharing {name}, residents x immigrants, min_bp {m}, chr {k}"
            S.same(g.ibd_segments(k, 0, r0, na, 0, r_imm, nb, min_bp=m), S.records(rect, min_bp=m, row_a0=r0, row_b0=r_imm), f"ibd_segments, residents x immigrants, min_bp {m}, chr {k}")
        for got, want, name in zip(g.ibd_sharing(k, 0, r0, nr, 0, r0, nr, min_bp=min_bp), sharing_from_runs(runs, min_bp), ("shared_bp", "n_seg", "max_seg")):
            assert np.array_equal(got, want), f"ibd_sharing {name}, square, min_bp {min_bp}, chr {k}"
        # ancestry
        bp, n_parts = g.ancestry_bp(0, k)
        assert np.array_equal(n_parts, np.diff(off.astype(np.int64)))
        want_bp = np.zeros((2 * n, M.N_POP), dtype=np.uint64)
        for r in range(2 * n):
            for x in parts[int(off[r]):int(off[r + 1])]:
                want_bp[r, int(x["root_population"])] += np.uint64(int(x["en"]) - int(x["st"]))
        assert np.array_equal(bp, want_bp), f"ancestry_bp chr {k}"
        # the .int text
        ids = np.arange(1000, 1000 + n, dtype=np.int64)
        want_txt = gpu_lib.dbg_format_interval_text_host(parts, off, ids, 22 - k, names)
        assert g.format_interval_text(0, k, 22 - k, ids=ids) == want_txt, f".int text chr {k}"
        w = gpu_lib.dbg_format_interval_text_host(parts, off, ids, 22 - k, names, header=False, ind_begin=N0, n_ind=N_IMM)
        assert g.format_interval_text(0, k, 22 - k, N0, N_IMM, header=False, ids=ids[N0:]) == w, f".int text of the immigrants chr {k}"
        # genotype counts and trait sums over the immigrants
        bits = M.raster_rows(M.IMMIGRANTS, k).astype(np.int64)
        geno = bits[0::2] + bits[1::2]                                # [N_IMM][L]
        het, hom = g.snp_genotype_counts(0, k, ind_begin=N0, n_ind=N_IMM)
        assert np.array_equal(het, (geno == 1).sum(axis=0)) and np.array_equal(hom, (geno == 2).sum(axis=0)), f"snp_genotype_counts chr {k}"
        trait = rs.randint(-2 ** 30, 2 ** 30 + 1, (3, N_IMM)).astype(np.int32)
        gsum, hetsum, n_het, n_hom = g.snp_trait_sums(0, k, trait, ind_begin=N0, n_ind=N_IMM)
        assert np.array_equal(gsum, trait.astype(np.int64) @ geno) and np.array_equal(hetsum, trait.astype(np.int64) @ (geno == 1).astype(np.int64)), f"snp_trait_sums chr {k}"
        assert np.array_equal(n_het, het) and np.array_equal(n_hom, hom)
    g.dbg_output_chunk(0)
    g.close()
