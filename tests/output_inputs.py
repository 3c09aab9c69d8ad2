"""What the genotype output calls return, by definition, and the populations they are pinned on.

The definitions are plain numpy on unpacked haplotype rows H[rows][L] (uint8 0/1, row 2i + h = haplotype h of individual i): the
SNP-major words of gev_download_snp_major, the PLINK .bed body of gev_format_bed, the .hap text of gev_format_hap_text, the sample
columns of gev_format_vcf_gt, the genotype columns of gev_format_ped_text and the interleaved matrix of gev_download_plink_matrix.
Nothing here calls a library; tests/test_outputs_cpu.py holds the definitions equal to the CPU oracle's own writers byte for byte.

The builders take a library object (the HIP library or the oracle) and drive it by the same statements: the same founder seeds, the
same glob seed stream, the same couples, the same moves.  A library that generates synthetic founders itself gets the seed, the other one
the same panel from tests/synth.py.  What a builder needs of GEV_SEG_CHUNKS is the caller's to set before it runs."""
import numpy as np

from geneevolve_amd.host import Simulation, SyntheticConfig, synthetic_random_mate
from tests.synth import synth_packed

AL0 = b"ACGT"
AL1 = b"TGCA"


# ---- definitions ------------------------------------------------------------------------------------------------------------------------
def unpack(words, L):
    """uint64 [rows][>= ceil(L / 64)] in the C-ABI packing (bit j of a row = locus j) -> uint8 [rows][L]"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :L]


def pack(bits01):
    """uint8 [rows][n] of 0/1 -> uint64 [rows][ceil(n / 64)], bit j of a row = column j, the bits behind column n - 1 zero"""
    b = np.asarray(bits01, dtype=np.uint8)
    wide = np.zeros((b.shape[0], -(-b.shape[1] // 64) * 64), dtype=np.uint8)
    wide[:, :b.shape[1]] = b
    return np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little")).view(np.uint64).reshape(b.shape[0], -1)


def allele_letters(L):
    """the two allele letters per SNP the .ped tests hand to format_ped_text"""
    return np.frombuffer(AL0, dtype=np.uint8)[np.arange(L) % 4], np.frombuffer(AL1, dtype=np.uint8)[(np.arange(L) // 3) % 4]


def snp_major_words(H, s0, ns):
    """uint64 [ns][ceil(rows / 64)]: bit r of row j = haplotype row r at SNP s0 + j"""
    return pack(H[:, s0:s0 + ns].T)


def bed_bytes(H, s0, ns):
    """PLINK .bed body of SNPs [s0, +ns), SNP-major, uint8 [ns * ceil(n / 4)]: individual i in bits 2 (i % 4).. of byte i // 4, A1 =
    allele 1: 00 = 1/1, 10 = heterozygous, 11 = 0/0, pad 00"""
    n = H.shape[0] // 2
    a, b = H[0::2, s0:s0 + ns].T, H[1::2, s0:s0 + ns].T             # [ns][n]
    code = np.where((a & b) == 1, 0, np.where((a ^ b) == 1, 2, 3)).astype(np.uint8)
    pad = (-n) % 4
    code = np.concatenate([code, np.zeros((ns, pad), dtype=np.uint8)], axis=1).reshape(ns, -1, 4)
    return (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).astype(np.uint8).ravel()


def hap_text(H, s0, ns):
    """.hap lines of SNPs [s0, +ns): per haplotype row its digit and a space, then a newline -> uint8 [ns * (2 rows + 1)]"""
    rows = H.shape[0]
    out = np.full((ns, 2 * rows + 1), ord(" "), dtype=np.uint8)
    out[:, 0:2 * rows:2] = H[:, s0:s0 + ns].T + ord("0")
    out[:, -1] = ord("\n")
    return out.ravel()


def vcf_gt(H, s0, ns):
    """sample columns of the VCF data lines of SNPs [s0, +ns): per individual "\\ta|b", then a newline -> uint8 [ns * (4 n + 1)]"""
    n = H.shape[0] // 2
    out = np.empty((ns, 4 * n + 1), dtype=np.uint8)
    out[:, 0:4 * n:4] = ord("\t"); out[:, 2:4 * n:4] = ord("|"); out[:, -1] = ord("\n")
    out[:, 1:4 * n:4] = H[0::2, s0:s0 + ns].T + ord("0")
    out[:, 3:4 * n:4] = H[1::2, s0:s0 + ns].T + ord("0")
    return out.ravel()


def ped_text(H, i0, ni, al0=None, al1=None):
    """genotype columns of the .ped lines of individuals [i0, +ni): per SNP " a b" (the allele letters of the two haplotypes, al1 where
    the bit is set; the digits 0 / 1 without letters), then a newline -> uint8 [ni * (4 L + 1)]"""
    L = H.shape[1]
    out = np.full((ni, 4 * L + 1), ord(" "), dtype=np.uint8)
    out[:, -1] = ord("\n")
    for hp in (0, 1):
        bits = H[2 * i0 + hp:2 * (i0 + ni):2, :]
        out[:, 1 + 2 * hp:4 * L:4] = bits + ord("0") if al0 is None else np.where(bits == 1, al1, al0)
    return out.ravel()


def plink_words(H, i0, ni):
    """matrix_plink_ped rows of individuals [i0, +ni): uint64 [ni][ceil(2 L / 64)], bit 2 * snp + hap"""
    L = H.shape[1]
    m = np.zeros((ni, 2 * L), dtype=np.uint8)
    m[:, 0::2] = H[2 * i0:2 * (i0 + ni):2]; m[:, 1::2] = H[2 * i0 + 1:2 * (i0 + ni):2]
    return pack(m) if ni else np.zeros((0, -(-2 * L // 64)), dtype=np.uint64)


# ---- conditions a population must meet, from a context's lists and rows ---------------------------------------------------------------------
def mutation_hits(ctx, pop, chr, pos, H, seg_loci):
    """mutations of the current generation's lists that sit on a SNP column, counted per segment of seg_loci loci and direction:
    -> int [n_segments][2], [g][0] = hits in segment g on a founder bit 1 (the row now shows 0), [g][1] = on a founder bit 0.
    A listed position flips its columns once, however often the list repeats it: the row's bit is the founder's, inverted"""
    muts, off = ctx.download_mutations(pop, chr)
    out = np.zeros((-(-len(pos) // seg_loci), 2), dtype=np.int64)
    for r in range(len(off) - 1):
        u = np.unique(muts[int(off[r]):int(off[r + 1])])
        lo, hi = np.searchsorted(pos, u, "left"), np.searchsorted(pos, u, "right")          # (the SNP grid is non-decreasing)
        for k in np.flatnonzero(hi > lo):
            for c in range(int(lo[k]), int(hi[k])):
                out[c // seg_loci, int(H[r, c])] += 1
    return out


def overlay_situations(ctx, pop, chr, pos, H):
    """(a) mutations at a SNP column whose founder bit was 1, (b) SNP positions mutated on both haplotypes of one individual, (c)
    positions repeated within one haplotype's list, (d) mutations at a position that two or more SNP columns share"""
    muts, off = ctx.download_mutations(pop, chr)
    a = b = c = d = 0
    for i in range(H.shape[0] // 2):
        lists = [muts[int(off[2 * i + h]):int(off[2 * i + h + 1])] for h in range(2)]
        for h, l in enumerate(lists):
            u, cnt = np.unique(l, return_counts=True)
            c += int((cnt > 1).sum())
            for x in u:
                cols = np.flatnonzero(pos == x)
                d += len(cols) > 1
                a += int((H[2 * i + h, cols] == 0).sum())
        b += int(np.isin(np.intersect1d(lists[0], lists[1]), pos).sum())
    return a, b, c, d


def units_named_twice(table, n_rows, nseg):
    """from the (row, segment) -> pool unit table of a generation: the units that two or more different rows name"""
    t = np.asarray(table).reshape(n_rows, nseg)
    pairs = np.unique(np.stack([t.ravel(), np.repeat(np.arange(n_rows), nseg)], axis=1), axis=0)      # (unit, row) once each
    _, rows_per_unit = np.unique(pairs[:, 0], return_counts=True)
    return int((rows_per_unit >= 2).sum())


# ---- populations ------------------------------------------------------------------------------------------------------------------------
class Built:
    """a population on one library: ctx, sim, and per (population, chromosome) the SNP count and positions"""

    def __init__(self, ctx, sim, sizes, pos):
        self.ctx, self.sim, self.sizes, self.pos = ctx, sim, list(sizes), pos

    def L(self, chr):
        return len(self.pos[chr])

    def rows(self, pop, chr):
        """the unpacked rows of the current generation as the context's download_haps has them"""
        return unpack(self.ctx.download_haps(pop, chr), self.L(chr))

    def close(self):
        self.ctx.close()


def _founders(ctx, pop, chr, nhap, L, seed):
    if ctx.L.exports("synth_founders"):
        ctx.synth_founders(pop, chr, nhap, seed)
    else:
        ctx.upload_founders(pop, chr, synth_packed(seed, nhap, L), L)


def _cv_founders(ctx, pop, phen, chr, nhap, ncv, seed):
    if ctx.L.exports("synth_cv_founders"):
        ctx.synth_cv_founders(pop, phen, chr, nhap, seed)
    else:
        ctx.upload_cv_founders(pop, phen, chr, synth_packed(seed, nhap, ncv), ncv)


def _bred_by_couples(lib, cfg, founder_seed, cv_seed, sim_seed, rng_seed, n_gen, before_reproduce):
    """one population, one chromosome: n_gen generations of synthetic_random_mate couples drawn from default_rng(rng_seed)"""
    n, L = cfg.n_ind, cfg.n_loci
    ctx = lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    _founders(ctx, 0, 0, 2 * n, L, founder_seed); _cv_founders(ctx, 0, 0, 0, 2 * n, len(cfg.cv[0][0][0]), cv_seed)
    sim = Simulation(ctx, sim_seed, 1, True)
    sim.ras_initial_human_gen0(0, n)
    rng = np.random.default_rng(rng_seed)
    for gen in range(1, n_gen + 1):
        sim.couples[0] = synthetic_random_mate(sim.sex[0], n, rng)
        if before_reproduce:
            before_reproduce(ctx, gen)
        sim.reproduce(0, gen)
    return Built(ctx, sim, [n], [cfg.snp_pos])


P1_N, P1_L, P1_GENS = 333, 5000, 3


def build_p1(lib, before_reproduce=None):
    """P1: 333 individuals x 5000 SNPs 400 bp apart, ~4 crossovers and ~100 new mutations per gamete, three generations.  A row is 640
    bytes: ten 64-byte segments of 512 loci under GEV_SEG_CHUNKS=4 (the last holds 392), three of 2048 under 16 (the last holds 904),
    one by default.  before_reproduce(ctx, gen) runs with the couples set, before generation gen is bred"""
    cfg = SyntheticConfig(P1_N, P1_L, chrom_bp=2_000_000, map_step=1000, rec_per_row=2e-3, mut_per_row=0.05, n_cv=10, seed=4)
    return _bred_by_couples(lib, cfg, 9, 10, 77, 0, P1_GENS, before_reproduce)


P2_N, P2_L, P2_GENS = 24, 33_000, 2


def build_p2(lib, before_reproduce=None):
    """P2: 24 individuals x 33 000 SNPs 100 bp apart, ~3 crossovers and ~66 new mutations per gamete, two generations: 48 rows (less than
    one 64-row transpose block) of 4125 bytes, more than 64 segments of 64 bytes"""
    cfg = SyntheticConfig(P2_N, P2_L, chrom_bp=3_300_000, map_step=1000, rec_per_row=1e-3, mut_per_row=0.02, n_cv=10, seed=8)
    return _bred_by_couples(lib, cfg, 21, 22, 78, 1, P2_GENS, before_reproduce)


P3_N, P3_L, P3_GENS = 150, 700, 8


def build_p3(lib):
    """P3: the population of test_counts_under_the_mutation_overlay: 150 individuals, 700 SNPs two base pairs apart on 1400 bp, 0.2
    mutations per 100 bp row and gamete, eight generations; SNP columns 10-12, 300-301 and 650-651 share a position.  A row is 128 bytes:
    two 64-byte segments of 512 loci under GEV_SEG_CHUNKS=4, columns 650-651 in the second"""
    cfg = SyntheticConfig(P3_N, P3_L, chrom_bp=1400, map_step=100, rec_per_row=0.05, mut_per_row=0.2, n_cv=8, seed=4)
    for k in (10, 11, 300, 650):
        cfg.snp_pos[k + 1] = cfg.snp_pos[k]
    ctx = lib.create(1, 1, 1)
    cfg.apply_static(ctx)
    _founders(ctx, 0, 0, 2 * P3_N, P3_L, 7); _cv_founders(ctx, 0, 0, 0, 2 * P3_N, 8, 8)
    sim = Simulation(ctx, 4, 1, True)
    sim.ras_initial_human_gen0(0, P3_N)
    for _ in range(P3_GENS):
        sim.next_generation_rm(0, P3_N)
    return Built(ctx, sim, [P3_N], [cfg.snp_pos])


P4_SIZES, P4_LS, P4_NCV = [37, 21], [1100, 700], 5
P4_MOVES = [(0, 7, 1), (0, 4, 1), (0, 0, 1)]


def p4_founder_seed(pop, chr):
    return 100 + 10 * pop + chr


def build_p4(lib):
    """P4: populations of 37 and 21 on chromosomes of 1100 and 700 SNPs (rows of 256 and 128 bytes), ~1.2 crossovers and ~6 new mutations
    per gamete, two generations each.  p4_move() and p4_breed() follow"""
    nchr, rs = len(P4_LS), np.random.RandomState(2718)
    ctx = lib.create(2, nchr, 1)
    R, step = 61, 1000
    bp = (500 + step * np.arange(R)).astype(np.uint64)
    prob, rate = np.r_[0.0, np.full(R - 1, 0.02)], np.r_[0.0, np.full(R - 1, 0.1)]
    pos = []
    for c in range(nchr):
        pos.append(np.sort(rs.choice(np.arange(600, 60000), P4_LS[c], replace=False)).astype(np.uint64))
        cvbp = np.sort(rs.choice(np.arange(600, 60000, 7), P4_NCV, replace=False)).astype(np.uint64)
        a, d = rs.randn(P4_NCV), rs.randn(P4_NCV)
        for p in range(2):
            ctx.set_rmap(p, c, bp, prob, step); ctx.set_mutmap(p, c, bp, rate); ctx.set_snps(p, c, pos[c])
            ctx.set_cvs(p, 0, c, cvbp, a, d, 0.0)
            _founders(ctx, p, c, 2 * P4_SIZES[p], P4_LS[c], p4_founder_seed(p, c))
            _cv_founders(ctx, p, 0, c, 2 * P4_SIZES[p], P4_NCV, 200 + 10 * p + c)
    sim = Simulation(ctx, 91, nchr, True)
    for p in range(2):
        sim.ras_initial_human_gen0(p, P4_SIZES[p])
    for _ in range(2):
        for p in range(2):
            sim.next_generation_rm(p, P4_SIZES[p])
    return Built(ctx, sim, P4_SIZES, pos)


def p4_move(built):
    """three individuals of population 0 move to population 1, as Simulation::ras_do_migration appends them"""
    built.sim.ras_do_migration(P4_MOVES)
    built.sizes = [built.sizes[0] - len(P4_MOVES), built.sizes[1] + len(P4_MOVES)]


def p4_breed(built):
    """one more generation of population 1"""
    built.sim.next_generation_rm(1, built.sizes[1])


def p4_founder_tiles(chr, s0, ns):
    """the founder panels of both root populations cut to SNPs [s0, +ns) of a chromosome, as materialize_pops / materialize_bed take them"""
    L = P4_LS[chr]
    return [pack(unpack(synth_packed(p4_founder_seed(p, chr), 2 * P4_SIZES[p], L), L)[:, s0:s0 + ns]) for p in range(2)]
