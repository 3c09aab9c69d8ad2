"""The genotype output calls (gev_download_snp_major, gev_format_hap_text, gev_format_vcf_gt, gev_format_bed, gev_format_ped_text,
gev_download_plink_matrix) on rows of many segments, most of them units named from an ancestor's row: the populations P1-P4 of
tests/output_inputs.py run through the HIP library and through the CPU oracle by the same statements; the truth of every call is the
numpy definition on the ORACLE's rows (tests/test_outputs_cpu.py holds the definitions equal to the oracle's own writers).  Every
comparison is byte or word equality (pytest -m gpu)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from tests import helpers
from tests import output_inputs as T

pytestmark = pytest.mark.gpu


@contextmanager
def seg_chunks(value):
    """GEV_SEG_CHUNKS for the contexts created inside (None: the default), put back afterwards"""
    old = os.environ.get("GEV_SEG_CHUNKS")
    if value is None:
        os.environ.pop("GEV_SEG_CHUNKS", None)
    else:
        os.environ["GEV_SEG_CHUNKS"] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("GEV_SEG_CHUNKS", None)
        else:
            os.environ["GEV_SEG_CHUNKS"] = old


def ind_ranges(n):
    """the whole population, ranges that start and end inside it, its last three, none"""
    return [(0, n), (1, 7), (n - 3, 3), (3, min(20, n - 3)), (5, 0)]


def truth(H, snp_ranges, ind_rgs):
    """what every call must return for the rows H, by definition, keyed as outputs() keys them"""
    L = H.shape[1]
    al0, al1 = T.allele_letters(L)
    want = {}
    for s0, ns in snp_ranges:
        want["snp_major", s0, ns] = T.snp_major_words(H, s0, ns)
        want["bed", s0, ns] = T.bed_bytes(H, s0, ns)
        want["hap_text", s0, ns] = T.hap_text(H, s0, ns)
        want["vcf_gt", s0, ns] = T.vcf_gt(H, s0, ns)
    for i0, ni in ind_rgs:
        want["plink", i0, ni] = T.plink_words(H, i0, ni)
        want["ped", i0, ni, False] = T.ped_text(H, i0, ni)
        want["ped", i0, ni, True] = T.ped_text(H, i0, ni, al0, al1)
    for v in want.values():
        v.setflags(write=False)
    return want


def padded(exact, wide):
    """a call with row_stride_words = needed + 3 into 0xFF bytes: the data words of the exact-width call, three zero pad words"""
    w = exact.shape[1]
    assert wide.shape == (exact.shape[0], w + 3) and np.array_equal(wide[:, :w], exact) and not wide[:, w:].any()


def outputs(g, pop, chr, L, snp_ranges, ind_rgs):
    """every output call on the ranges -> all the bytes they returned; the row matrices also with a row stride three words wider"""
    al0, al1 = T.allele_letters(L)
    got = {}
    for s0, ns in snp_ranges:
        got["snp_major", s0, ns] = sm = g.download_snp_major(pop, chr, s0, ns)
        padded(sm, g.download_snp_major(pop, chr, s0, ns, stride_words=sm.shape[1] + 3))
        got["bed", s0, ns] = g.format_bed(pop, chr, s0, ns)
        got["hap_text", s0, ns] = g.format_hap_text(pop, chr, s0, ns)
        got["vcf_gt", s0, ns] = g.format_vcf_gt(pop, chr, s0, ns)
    for i0, ni in ind_rgs:
        got["plink", i0, ni] = pm = g.download_plink_matrix(pop, chr, i0, ni)
        padded(pm, g.download_plink_matrix(pop, chr, i0, ni, stride_words=pm.shape[1] + 3))
        for letters in (False, True):
            got["ped", i0, ni, letters] = g.format_ped_text(pop, chr, al0 if letters else None, al1 if letters else None, i0, ni)
    return got


def same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what}: {k} is {got[k].dtype}{got[k].shape}"
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.argwhere(got[k] != want[k])[:5].tolist()}"


def rows_equal_the_oracle(g, o, pop, chr, what):
    """gev_download_haps against the oracle's: whole, rows [5, +30), and both with a row stride three words wider -> the oracle's words"""
    words = o.download_haps(pop, chr)
    got = g.download_haps(pop, chr)
    assert np.array_equal(got, words), f"{what}: dense genotypes differ from the oracle's"
    sub = g.download_haps(pop, chr, 5, 30)
    assert np.array_equal(sub, words[5:35]), f"{what}: rows [5, 35)"
    padded(words, g.download_haps(pop, chr, stride_words=words.shape[1] + 3))
    padded(sub, g.download_haps(pop, chr, 5, 30, stride_words=words.shape[1] + 3))
    return words


def whole_and_chunked(g, o, pop, chr, L, snp_ranges, ind_rgs, what, want=None):
    """the rows against the oracle's, then every call against the definitions on the oracle's rows: in the staging passes the byte
    budgets give (one per call at these sizes) and with gev_dbg_output_chunk(7): SNP passes of 64 from starts that fall inside words and
    segments, 7 rows and 7 individuals per pass; byte for byte the same -> the truth"""
    words = rows_equal_the_oracle(g, o, pop, chr, what)
    if want is None:
        want = truth(T.unpack(words, L), snp_ranges, ind_rgs)
    whole = outputs(g, pop, chr, L, snp_ranges, ind_rgs)
    same(whole, want, what)
    g.dbg_output_chunk(7)
    try:
        rows_equal_the_oracle(g, o, pop, chr, f"{what}, output chunk 7")
        chunked = outputs(g, pop, chr, L, snp_ranges, ind_rgs)
    finally:
        g.dbg_output_chunk(0)
    same(chunked, want, f"{what}, output chunk 7")
    same(chunked, whole, f"{what}, output chunk 7 against one pass")
    return want


class Sharing:
    """the unit table of a chromosome read before the last generation is bred and after: how its rows share pool units"""

    def __init__(self, last_gen):
        self.last_gen, self.before = last_gen, None

    def before_reproduce(self, ctx, gen):
        if gen == self.last_gen:
            _, _, n_slots, tab, nseg = ctx.plane_ptr(0, 0)
            self.before = helpers.read_device_u32(tab, n_slots * nseg)

    def figures(self, ctx):
        """-> (unit bytes, segments per row, table entries that name a unit of the parents' generation, units that two or more rows of
        the current generation name)"""
        _, unit_bytes, n_slots, tab, nseg = ctx.plane_ptr(0, 0)
        after = helpers.read_device_u32(tab, n_slots * nseg)
        return unit_bytes, nseg, int(np.isin(after, self.before).sum()), T.units_named_twice(after, n_slots, nseg)


# ---- P1: many segments ---------------------------------------------------------------------------------------------------------------------
P1_SNPS = [(0, T.P1_L), (63, 1), (64, 1), (T.P1_L - 1, 1), (70, 999), (511, 2), (512, 512), (4608, 392)]


@pytest.fixture(scope="module")
def p1_oracle(oracle_lib):
    """P1 on the oracle and the truth of every call, computed once for the three segment sizes and left unchanged"""
    o = T.build_p1(oracle_lib)
    want = truth(o.rows(0, 0), P1_SNPS, ind_ranges(T.P1_N))
    yield o, want
    o.close()


@pytest.mark.parametrize("chunks,unit_bytes,nseg", [(4, 64, 10), (16, 256, 3), (None, 1024, 1)], ids=["10 segments", "3 segments", "1 segment"])
def test_p1_rows_of_many_segments(gpu_lib, p1_oracle, chunks, unit_bytes, nseg):
    """333 x 5000, three generations, under GEV_SEG_CHUNKS = 4 (ten 64-byte segments of 512 loci per row, the last holds 392), 16
    (three segments of 2048, the last holds 904) and the default (one segment: the control).  SNP ranges: everything, one SNP either
    side of a word edge, the last SNP, (70, 999), (511, 2) across a segment edge, (512, 512) exactly one segment, (4608, 392) the partial
    last segment.  Measured: of the 6660 (1998) table entries of the last generation 4483 (572) name a unit of the parents' generation,
    and 1110 (83) units are named by two or more of its rows; with one segment per row 10 of 666 and none."""
    o, want = p1_oracle
    sharing = Sharing(T.P1_GENS)
    with seg_chunks(chunks):
        g = T.build_p1(gpu_lib, sharing.before_reproduce)
    try:
        fig = sharing.figures(g.ctx)
        print(f"P1, GEV_SEG_CHUNKS={chunks}: unit bytes {fig[0]}, segments per row {fig[1]}, entries naming a parental unit {fig[2]}, units named by two rows {fig[3]}")
        assert fig[:2] == (unit_bytes, nseg)
        if nseg > 1:
            assert fig[2] > 0, "n_shared: no table entry of the last generation names a parental unit"
            assert fig[3] > 0, "no pool unit is named by two different rows of the current generation"
        whole_and_chunked(g.ctx, o.ctx, 0, 0, T.P1_L, P1_SNPS, ind_ranges(T.P1_N), f"P1, {nseg} segments per row", want)
    finally:
        g.close()


# ---- P2: the segment limit -----------------------------------------------------------------------------------------------------------------
def test_p2_more_than_64_segments_asked_for(gpu_lib, oracle_lib):
    """24 x 33 000 under GEV_SEG_CHUNKS=4, two generations: 48 rows, less than one 64-row transpose block; a row of 4125 bytes (264
    chunks with its padding) would be 66 segments of 64 bytes, so the library doubles the segment: gev_plane_ptr reports 33 segments of
    128 bytes = 1024 loci.  SNP ranges: everything, (1023, 2) and (1000, 100) across the first segment edge, (1024, 1024) the second
    segment, the last SNP.  Measured: of the 1584 table entries of the last generation 1434 name a unit of the parents' generation, and
    384 units are named by two or more of its rows."""
    snps = [(0, T.P2_L), (1023, 2), (1000, 100), (1024, 1024), (T.P2_L - 1, 1)]
    o = T.build_p2(oracle_lib)
    sharing = Sharing(T.P2_GENS)
    with seg_chunks(4):
        g = T.build_p2(gpu_lib, sharing.before_reproduce)
    try:
        fig = sharing.figures(g.ctx)
        print(f"P2: unit bytes {fig[0]}, segments per row {fig[1]}, entries naming a parental unit {fig[2]}, units named by two rows {fig[3]}")
        assert fig[:2] == (128, 33)
        assert fig[2] > 0, "n_shared: no table entry of the last generation names a parental unit"
        assert fig[3] > 0, "no pool unit is named by two different rows of the current generation"
        whole_and_chunked(g.ctx, o.ctx, 0, 0, T.P2_L, snps, ind_ranges(T.P2_N), "P2")
    finally:
        g.close(); o.close()


# ---- P3: the mutation overlay on shared positions ------------------------------------------------------------------------------------------
def test_p3_overlay_with_shared_positions(gpu_lib, oracle_lib):
    """the population of test_counts_under_the_mutation_overlay under GEV_SEG_CHUNKS=4: two 64-byte segments per row, the SNP columns
    650-651 that share a position in the second.  tests/test_outputs_cpu.py asserts its situations on the oracle ((a) 421, (b) 12, (c)
    12, (d) 11, mutation hits on founder bits of both values in both segments); here they are asserted again from the device's own
    lists.  SNP ranges: everything, the three columns of one position, the middle one alone, ranges that begin and end between columns
    of a shared position"""
    snps = [(0, T.P3_L), (10, 3), (11, 1), (301, 350), (129, 571)]
    o = T.build_p3(oracle_lib)
    with seg_chunks(4):
        g = T.build_p3(gpu_lib)
    try:
        assert g.ctx.plane_ptr(0, 0)[1] == 64 and g.ctx.plane_ptr(0, 0)[4] == 2
        whole_and_chunked(g.ctx, o.ctx, 0, 0, T.P3_L, snps, ind_ranges(T.P3_N), "P3")
        H = o.rows(0, 0)
        sit = T.overlay_situations(g.ctx, 0, 0, g.pos[0], H)
        hits = T.mutation_hits(g.ctx, 0, 0, g.pos[0], H, 512)
        print(f"P3: situations (a)-(d) {sit}, hits per segment [founder 1, founder 0] {hits.tolist()}")
        assert all(x >= 1 for x in sit) and (hits >= 1).all()
    finally:
        g.close(); o.close()


# ---- P4: two populations, two chromosomes, a migration -------------------------------------------------------------------------------------
def p4_snps(L):
    return [(0, L), (63, 1), (64, 1), (511, 2), (500, 150), (L - 1, 1)]


def p4_check(g, o, pops, what):
    """every call for the populations given and both chromosomes, and the tiles from the founder panels against the same truth"""
    for p in pops:
        n = o.sizes[p]
        assert g.ctx.pop_size(p) == o.ctx.pop_size(p) == n
        for c in range(2):
            L = T.P4_LS[c]
            label = f"P4 {what}, population {p} chromosome {c}"
            whole_and_chunked(g.ctx, o.ctx, p, c, L, p4_snps(L), ind_ranges(n), label)
            H = o.rows(p, c)
            for s0, ns in ((0, L), (500, 150), (511, 2)):
                tiles = T.p4_founder_tiles(c, s0, ns)
                assert np.array_equal(g.ctx.materialize_pops(p, c, tiles, 0, None, s0, ns), T.pack(H[:, s0:s0 + ns])), f"{label}: materialize_pops SNPs [{s0},+{ns})"
                assert np.array_equal(g.ctx.materialize_pops(p, c, tiles, 3, 11, s0, ns), T.pack(H[3:14, s0:s0 + ns])), f"{label}: materialize_pops rows [3,14) SNPs [{s0},+{ns})"
                assert np.array_equal(g.ctx.materialize_bed(p, c, tiles, s0, ns), T.bed_bytes(H, s0, ns)), f"{label}: materialize_bed SNPs [{s0},+{ns})"


def test_p4_two_populations_behind_a_migration(gpu_lib, oracle_lib):
    """populations of 37 and 21 on chromosomes of 1100 and 700 SNPs under GEV_SEG_CHUNKS=4: rows of 256 and 128 bytes, which
    gev_plane_ptr reports as four and two 64-byte segments (1100 loci fill three; the fourth is the padding of the row to 128 bytes).
    Two generations each; three individuals move from population 0 to 1 and the first output call on population 1 comes directly behind
    the move, so it materialises the pending order on rows of several segments; one more generation of population 1.  Then the largest
    request, the smallest and the largest again, which must return the first call's bytes: the staging buffers are shared across calls
    of different sizes"""
    o = T.build_p4(oracle_lib)
    with seg_chunks(4):
        g = T.build_p4(gpu_lib)
    try:
        for p in range(2):
            assert [g.ctx.plane_ptr(p, c)[1] for c in range(2)] == [64, 64] and [g.ctx.plane_ptr(p, c)[4] for c in range(2)] == [4, 2]
        p4_check(g, o, (0, 1), "before the move")
        T.p4_move(g); T.p4_move(o)
        first = g.ctx.download_snp_major(1, 0)                               # before anything else has asked for population 1's rows
        assert np.array_equal(first, T.snp_major_words(o.rows(1, 0), 0, T.P4_LS[0])), "the first call directly behind the move"
        p4_check(g, o, (1, 0), "behind the move")
        T.p4_breed(g); T.p4_breed(o)
        p4_check(g, o, (1, 0), "after the next generation")
        # the staging buffers across calls of different sizes
        L, n = T.P4_LS[0], o.sizes[0]
        al0, al1 = T.allele_letters(L)
        calls = {
            "snp_major": lambda big: g.ctx.download_snp_major(0, 0) if big else g.ctx.download_snp_major(1, 1, 5, 1),
            "hap_text": lambda big: g.ctx.format_hap_text(0, 0) if big else g.ctx.format_hap_text(1, 1, 5, 1),
            "vcf_gt": lambda big: g.ctx.format_vcf_gt(0, 0) if big else g.ctx.format_vcf_gt(1, 1, 5, 1),
            "bed": lambda big: g.ctx.format_bed(0, 0) if big else g.ctx.format_bed(1, 1, 5, 1),
            "plink": lambda big: g.ctx.download_plink_matrix(0, 0) if big else g.ctx.download_plink_matrix(1, 1, 5, 1),
            "ped": lambda big: g.ctx.format_ped_text(0, 0, al0, al1) if big else g.ctx.format_ped_text(1, 1, None, None, 5, 1),
            "haps": lambda big: g.ctx.download_haps(0, 0) if big else g.ctx.download_haps(1, 1, 5, 1),
        }
        H0, H1 = o.rows(0, 0), o.rows(1, 1)
        large = {"snp_major": T.snp_major_words(H0, 0, L), "hap_text": T.hap_text(H0, 0, L), "vcf_gt": T.vcf_gt(H0, 0, L), "bed": T.bed_bytes(H0, 0, L),
                 "plink": T.plink_words(H0, 0, n), "ped": T.ped_text(H0, 0, n, al0, al1), "haps": T.pack(H0)}
        small = {"snp_major": T.snp_major_words(H1, 5, 1), "hap_text": T.hap_text(H1, 5, 1), "vcf_gt": T.vcf_gt(H1, 5, 1), "bed": T.bed_bytes(H1, 5, 1),
                 "plink": T.plink_words(H1, 5, 1), "ped": T.ped_text(H1, 5, 1), "haps": T.pack(H1[5:6])}
        for name, call in calls.items():
            a, b, c = call(True), call(False), call(True)
            assert np.array_equal(a, large[name]) and np.array_equal(b, small[name]), f"{name}: largest, then smallest request"
            assert np.array_equal(c, a), f"{name}: the largest request repeated behind the smallest"
    finally:
        g.close(); o.close()
