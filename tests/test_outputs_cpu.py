"""The truth of tests/test_gpu_outputs_segments.py, pinned before a GPU is involved: the populations P1-P4 of tests/output_inputs.py built
on the CPU oracle meet the conditions the GPU tests rely on, and the numpy definitions of the output formats reproduce the oracle's own
format_hap_text, format_vcf_gt, format_bed, format_ped_text and download_plink_matrix byte for byte (pytest -m "not gpu")."""
import numpy as np

from tests import output_inputs as T


def definitions_equal_the_oracle(built, pop, chr, snp_ranges=(), ind_ranges=()):
    """whole ranges, and the sub-ranges given, of every writer the oracle has against the definitions on its own rows"""
    o, L, n = built.ctx, built.L(chr), built.sizes[pop]
    assert o.pop_size(pop) == n
    H = built.rows(pop, chr)
    assert H.shape == (2 * n, L)
    al0, al1 = T.allele_letters(L)
    for s0, ns in [(0, L), *snp_ranges]:
        what = f"population {pop} chromosome {chr} SNPs [{s0},+{ns})"
        assert np.array_equal(o.format_hap_text(pop, chr, s0, ns), T.hap_text(H, s0, ns)), what
        assert np.array_equal(o.format_vcf_gt(pop, chr, s0, ns), T.vcf_gt(H, s0, ns)), what
        assert np.array_equal(o.format_bed(pop, chr, s0, ns), T.bed_bytes(H, s0, ns)), what
    for i0, ni in [(0, n), *ind_ranges]:
        what = f"population {pop} chromosome {chr} individuals [{i0},+{ni})"
        assert np.array_equal(o.download_plink_matrix(pop, chr, i0, ni), T.plink_words(H, i0, ni)), what
        assert np.array_equal(o.format_ped_text(pop, chr, None, None, i0, ni), T.ped_text(H, i0, ni)), what
        assert np.array_equal(o.format_ped_text(pop, chr, al0, al1, i0, ni), T.ped_text(H, i0, ni, al0, al1)), what
    return H


def test_definitions_on_a_matrix_written_out_by_hand():
    """three individuals, five SNPs: every format spelled out"""
    H = np.array([[1, 0, 1, 0, 1],
                  [1, 0, 0, 1, 1],
                  [0, 0, 1, 1, 0],
                  [0, 1, 1, 0, 0],
                  [1, 1, 0, 0, 1],
                  [0, 1, 0, 1, 1]], dtype=np.uint8)
    assert T.snp_major_words(H, 1, 3).tolist() == [[0b111000], [0b001101], [0b100110]]
    assert T.bed_bytes(H, 0, 2).tolist() == [0b00101100, 0b00001011]                     # 1/1 0/0 het, then 0/0 het 1/1; the pad is 00
    assert T.hap_text(H, 0, 2).tobytes() == b"1 1 0 0 1 0 \n0 0 0 1 1 1 \n"
    assert T.vcf_gt(H, 3, 2).tobytes() == b"\t0|1\t1|0\t0|1\n\t1|1\t0|0\t1|1\n"
    assert T.ped_text(H, 1, 2).tobytes() == b" 0 0 0 1 1 1 1 0 0 0\n 1 0 1 1 0 0 0 1 1 1\n"
    al0, al1 = T.allele_letters(5)
    assert (al0.tobytes(), al1.tobytes()) == (b"ACGTA", b"TTTGG")
    assert T.ped_text(H, 0, 1, al0, al1).tobytes() == b" T T C C T G T G G G\n"
    assert T.ped_text(H, 2, 0).size == 0 and T.plink_words(H, 2, 0).shape == (0, 1)
    assert T.plink_words(H, 0, 3).tolist() == [[0b1110010011], [0b0001111000], [0b1110001101]]
    assert T.unpack(T.pack(H), 5).tolist() == H.tolist()
    assert T.units_named_twice([5, 6, 7, 5, 8, 7, 9, 9, 1], 3, 3) == 2                    # units 5 and 7; 9 twice in one row does not count


def test_p1_on_the_oracle(oracle_lib):
    """mutation hits on SNP columns per segment as [on a founder 1, on a founder 0], measured: ten segments of 512 loci: first [5, 16],
    sixth [8, 20], last [6, 25] (none of the ten without either); three of 2048: [22, 96], [29, 76], [18, 51]"""
    b = T.build_p1(oracle_lib)
    H = definitions_equal_the_oracle(b, 0, 0)
    for seg_loci, nseg in ((512, 10), (2048, 3)):
        hits = T.mutation_hits(b.ctx, 0, 0, b.pos[0], H, seg_loci)
        print(f"P1, segments of {seg_loci} loci: hits [founder 1, founder 0] per segment {hits.tolist()}")
        assert len(hits) == nseg
        for g in (0, nseg // 2, nseg - 1):
            assert hits[g, 0] >= 1 and hits[g, 1] >= 1, (seg_loci, g, hits.tolist())
    b.close()


def test_p2_on_the_oracle(oracle_lib):
    """mutation hits on SNP columns, measured: 5 on a founder 1 and 18 on a founder 0, in 15 of the 33 segments of 1024 loci, the first
    and the last among them"""
    b = T.build_p2(oracle_lib)
    H = definitions_equal_the_oracle(b, 0, 0, ind_ranges=[(1, 7)])
    hits = T.mutation_hits(b.ctx, 0, 0, b.pos[0], H, 1024)
    print(f"P2, segments of 1024 loci: hits [founder 1, founder 0] {hits.sum(axis=0).tolist()} in {int((hits.sum(axis=1) > 0).sum())} of {len(hits)} segments")
    assert len(hits) == 33 and hits[0].sum() >= 1 and hits[-1].sum() >= 1
    b.close()


def test_p3_on_the_oracle(oracle_lib):
    """(a) cleared founder bits 421, (b) both haplotypes 12, (c) repeated positions 12, (d) shared positions 11, as
    test_counts_under_the_mutation_overlay has them; hits per segment of 512 loci as [on a founder 1, on a founder 0]: [313, 870],
    [108, 300]"""
    b = T.build_p3(oracle_lib)
    H = definitions_equal_the_oracle(b, 0, 0, snp_ranges=[(10, 3), (11, 1), (301, 350), (129, 571)], ind_ranges=[(1, 7), (147, 3), (3, 20), (5, 0)])
    sit = T.overlay_situations(b.ctx, 0, 0, b.pos[0], H)
    hits = T.mutation_hits(b.ctx, 0, 0, b.pos[0], H, 512)
    print(f"P3: (a) cleared founder bits {sit[0]}, (b) both haplotypes {sit[1]}, (c) repeated positions {sit[2]}, (d) shared positions {sit[3]}; hits {hits.tolist()}")
    assert all(x >= 1 for x in sit), sit
    assert hits.shape == (2, 2) and (hits >= 1).all(), hits.tolist()
    b.close()


def test_p4_on_the_oracle(oracle_lib):
    """both populations and chromosomes before the move, behind it, and after one more generation of population 1, which then
    holds rows of either root population"""
    b = T.build_p4(oracle_lib)

    def all_of_them():
        for p in range(2):
            for c in range(2):
                L, n = b.L(c), b.sizes[p]
                H = definitions_equal_the_oracle(b, p, c, snp_ranges=[(511, 2), (L - 1, 1)], ind_ranges=[(1, 7), (n - 3, 3), (5, 0)])
                tiles = T.p4_founder_tiles(c, 0, L)
                assert np.array_equal(b.ctx.materialize_pops(p, c, tiles), T.pack(H)), (p, c)
    all_of_them()
    T.p4_move(b)
    assert b.sizes == [34, 24]
    all_of_them()
    T.p4_breed(b)
    all_of_them()
    for c in range(2):
        parts, off = b.ctx.download_intervals(1, c)
        roots = [set(parts["root_population"][int(off[r]):int(off[r + 1])].tolist()) for r in range(len(off) - 1)]
        assert {0} in roots and {1} in roots, "population 1 was meant to hold rows of either root population: a migrant has bred"
    b.close()
