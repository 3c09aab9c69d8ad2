"""Hand-built migrant records: the setting, the immigrants and the plain truth the CPU and GPU tests share (test_migrant_inputs_cpu.py,
test_gpu_migrant_import.py).

Three populations on two chromosomes, two phenotypes.  Founder panels and CV founders are UPLOADED, so every bit is known in numpy (the
genotype panels are tests.synth's, which gev_dbg_verify_planes can regenerate on the device; the CV founders are plain random bits).
Chromosome 0 has 600 loci on a 2 Mb map: 31 position ranges of 2^16 bp at the default width (4 of 2^19 bp under GEV_LIST_SEGS=5);
chromosome 1 has 130 loci on a 60 kb map.  The CV files of both phenotypes are not in position order and hold one pair of equal
positions per chromosome.

The immigrants are lists no simulation of this size produces: rows of hundreds of parts, many parts inside one range between two empty
ranges, parts and zero-length parts on range edges and at the last map position, mutation lists of hundreds of positions with entries on
range edges, part boundaries, SNPs and CVs.  `assert_coverage` (run on import of this module) asserts every such property, so that a
later edit cannot quietly thin them out.

The truth functions (`raster_rows`, `raster_cv`) are plain loops: the founder bit under the part that covers the position, XOR
membership in the row's mutation list.  tests/test_migrant_inputs_cpu.py holds them equal to the oracle, which is what licenses them.

One crafted input had to give way to the oracle: a mutation ON the last map position.  Parts are [st, en) and end at the last map
position, so no part covers it, the reference's ras_add_mutation (src/Simulation.cpp:2526) drops a new mutation there, and the oracle's
lists (mutations kept with their part) cannot hold one.  The last mutated position is therefore the last one a part covers,
`last map position - 1`, and helpers.encode_oracle_record refuses anything else."""
import numpy as np

from geneevolve_amd.capi import PART_DTYPE, pack_rows
from tests.synth import synth_bits

N_POP, NCHR, NPHEN = 3, 2, 2
RESIDENTS = [14, 12, 16]                                     # individuals per population at generation 0 (= founders / 2)
LS = [600, 130]
BP0 = [1000, 500]
MAP_STEP = [20_000, 1000]
MAP_ROWS = [101, 61]
BP_END = [BP0[k] + MAP_STEP[k] * (MAP_ROWS[k] - 1) for k in range(NCHR)]          # 2 001 000, 60 500
SPAN = [(BP0[k], BP_END[k]) for k in range(NCHR)]
LGW = 16                                                     # chromosome 0, default width: (2 000 000 >> 16) + 1 = 31 ranges
N_RANGES = ((BP_END[0] - BP0[0]) >> LGW) + 1
CROWDED = 7                                                  # the range that holds >= 40 parts of one row; ranges 6 and 8 hold none of that row


def edge(t):
    """first position of range t of chromosome 0 at the default width"""
    return BP0[0] + (t << LGW)


def founder_seed(p, k):
    return 100 + 10 * p + k


def n_founders(p):
    return 2 * RESIDENTS[p]


_rs = np.random.RandomState(20261)

# ---- maps: hot around the crowded range of chromosome 0 (crossovers and new mutations fall between its parts), mild elsewhere
RMAP_BP = [(BP0[k] + MAP_STEP[k] * np.arange(MAP_ROWS[k])).astype(np.uint64) for k in range(NCHR)]
RMAP_PROB, MUT_RATE = [], []
for _k in range(NCHR):
    prob = np.r_[0.0, np.full(MAP_ROWS[_k] - 1, 0.02)]; rate = np.r_[0.0, np.full(MAP_ROWS[_k] - 1, 0.03)]
    if _k == 0:
        hot = (RMAP_BP[0] + MAP_STEP[0] > edge(CROWDED)) & (RMAP_BP[0] < edge(CROWDED + 1))
        prob[hot] = 0.6; rate[np.flatnonzero(hot) + 1] = 0.6
        prob[0] = 0.0
    RMAP_PROB.append(prob); MUT_RATE.append(rate)

# ---- CVs: file order is not position order, one pair of equal positions per (phenotype, chromosome)
N_CV = [[37, 5], [33, 3]]                                    # [phenotype][chromosome]
CV_PAIR_POS = [edge(CROWDED) + 3000, 30_011]                 # the pair of equal positions of phenotype 0, per chromosome
CV_POS, CV_A, CV_D = [], [], []                              # CV_POS[p][k]; CV_A[pop][p][k] (effects differ per population: A/D reads the root population)
for _p in range(NPHEN):
    CV_POS.append([])
    for _k in range(NCHR):
        c = N_CV[_p][_k]
        pos = _rs.choice(np.arange(BP0[_k] + 5, BP_END[_k] - 5, 7), c - 2, replace=False).astype(np.uint64)
        pair = CV_PAIR_POS[_k] + 13 * _p
        pos = np.r_[pos[:c // 2], np.uint64(pair), pos[c // 2:], np.uint64(pair)].astype(np.uint64)      # the pair is not adjacent in the file
        if _k == 0 and _p == 0:
            pos[1] = edge(12)                                # a CV on a range edge
        assert len(pos) == c and len(np.unique(pos)) == c - 1 and (np.diff(pos.astype(np.int64)) < 0).any()
        CV_POS[-1].append(pos)
for _pop in range(N_POP):
    CV_A.append([[_rs.randn(N_CV[p][k]) for k in range(NCHR)] for p in range(NPHEN)])
    CV_D.append([[_rs.randn(N_CV[p][k]) for k in range(NCHR)] for p in range(NPHEN)])
CV_VD = 0.3

# ---- SNPs: 600 / 130 sorted positions, with the first map position, range edges and their neighbours, and the last covered position
SNP_POS = []
for _k in range(NCHR):
    special = [BP0[_k], BP_END[_k] - 1]
    if _k == 0:
        special += [edge(5) - 1, edge(5), edge(5) + 1, edge(9), edge(12), edge(CROWDED), edge(CROWDED) + 700, edge(30), edge(30) + 1, int(CV_POS[0][0][3])]
    rest = _rs.choice(np.setdiff1d(np.arange(BP0[_k] + 1, BP_END[_k] - 1), special), LS[_k] - len(special), replace=False)
    SNP_POS.append(np.sort(np.r_[special, rest]).astype(np.uint64))
    assert len(np.unique(SNP_POS[-1])) == LS[_k]

# ---- founders: FOUNDERS[k][rp] bits [2 * RESIDENTS[rp]][L]; CV_FOUNDERS[p][k][rp] bits [..][C] in file order
FOUNDERS = [[synth_bits(founder_seed(rp, k), n_founders(rp), LS[k]) for rp in range(N_POP)] for k in range(NCHR)]
CV_FOUNDERS = [[[(_rs.rand(n_founders(rp), N_CV[p][k]) < 0.4).astype(np.uint8) for rp in range(N_POP)] for k in range(NCHR)] for p in range(NPHEN)]


# ---- the immigrants ----------------------------------------------------------------------------------------------------------------
def tiled(k, cuts, labels):
    """parts [(st, en, hap_index, root_population)] from ascending cuts (first = first map position, last = last map position; equal
    neighbours give zero-length parts) and one (hap_index, root_population) per part"""
    assert len(labels) == len(cuts) - 1 and cuts[0] == BP0[k] and cuts[-1] == BP_END[k]
    return [(int(cuts[q]), int(cuts[q + 1]), int(labels[q][0]), int(labels[q][1])) for q in range(len(labels))]


def _labels(rs, n, first=None):
    """n labels over all three root populations; neighbours differ (a part boundary is then a change of ancestry)"""
    out = [first] if first is not None else []
    while len(out) < n:
        rp = int(rs.randint(N_POP)); lab = (int(rs.randint(n_founders(rp))), rp)
        if not out or out[-1] != lab:
            out.append(lab)
    return out


def _random_row(rs, k, n_parts, n_muts, cuts_extra=(), muts_extra=()):
    inner = set(int(x) for x in cuts_extra)
    while len(inner) < n_parts - 1:
        inner.add(int(rs.randint(BP0[k] + 1, BP_END[k])))
    cuts = [BP0[k]] + sorted(inner) + [BP_END[k]]
    muts = set(int(x) for x in muts_extra)
    while len(muts) < n_muts:
        muts.add(int(rs.randint(BP0[k], BP_END[k])))
    return tiled(k, cuts, _labels(rs, len(cuts) - 1)), sorted(muts)


def _build():
    rs = np.random.RandomState(77003)
    last = [(n_founders(rp) - 1, rp) for rp in range(N_POP)]           # the last founder of each root population
    first = [(0, rp) for rp in range(N_POP)]
    E = edge
    # 0: one-part rows, no mutation anywhere; hap_index 0 and the last founder
    one = {"sex": 1, "chr": [[(tiled(k, [BP0[k], BP_END[k]], [first[0]]), []), (tiled(k, [BP0[k], BP_END[k]], [last[2]]), [])] for k in range(NCHR)]}
    # 1: chromatid 0: 320 parts and 330 mutations over the whole map; chromatid 1: 45 parts start inside the crowded range, none in its neighbours
    long_row = _random_row(rs, 0, 320, 330, muts_extra=[BP0[0], BP_END[0] - 1, E(3), E(CROWDED), int(SNP_POS[0][17]), int(CV_POS[1][0][4])])
    inside = sorted(set(int(x) for x in rs.randint(E(CROWDED) + 1, E(CROWDED + 1) - 1, 60)))[:44]
    cuts = [BP0[0], E(3) + 17, E(CROWDED)] + inside + [E(10) + 5, E(20), BP_END[0]]
    crowded = (tiled(0, cuts, _labels(rs, len(cuts) - 1, first=last[0])),
               sorted(set([E(CROWDED) + 700, inside[3], inside[20]] + [int(x) for x in rs.randint(E(CROWDED), E(CROWDED + 1), 25)])))
    many = {"sex": 2, "chr": [[long_row, crowded], [_random_row(rs, 1, 9, 6), _random_row(rs, 1, 1, 0)]]}
    # 2: range edges.  chromatid 0: parts that start one bp in front of, on and one bp behind an edge, the same in the last range, a
    # zero-length part on an edge, one at the last map position; mutations on an edge, a part boundary, a SNP, a CV, the CV pair of equal
    # positions, the first map position and the last covered one
    cuts = [BP0[0], E(5) - 1, E(5), E(5) + 1, E(9), E(9), E(12), E(12) + 1, E(17) - 1, E(30) - 1, E(30), E(30) + 1, E(30) + 900, BP_END[0], BP_END[0]]
    labels = [first[1], last[1], first[2], last[0], first[0], last[2], first[1], last[1], first[2], last[2], first[0], last[0], first[1], last[1]]
    muts = sorted({BP0[0], E(5), E(9), E(12) + 1, int(SNP_POS[0][100]), int(SNP_POS[0][599]), int(CV_POS[0][0][7]), CV_PAIR_POS[0], CV_PAIR_POS[0] + 13, E(12), BP_END[0] - 1})
    edges0 = (tiled(0, cuts, labels), muts)
    # chromatid 1: two zero-length parts on one edge, zero-length parts in front of the last range's edge and at the last map position
    cuts = [BP0[0], E(1), E(1), E(1), E(2) + 1, E(29), E(30), E(30), BP_END[0] - 1, BP_END[0], BP_END[0]]
    edges1 = (tiled(0, cuts, _labels(rs, len(cuts) - 1, first=first[2])), [E(1), E(2), E(30), BP_END[0] - 1])
    c1 = [BP0[1], BP0[1] + (5 << 11), BP0[1] + (5 << 11), BP0[1] + (5 << 11) + 1, CV_PAIR_POS[1], BP_END[1], BP_END[1]]
    onedge = {"sex": 1, "chr": [[edges0, edges1], [(tiled(1, c1, _labels(rs, len(c1) - 1)), sorted({BP0[1], CV_PAIR_POS[1], int(SNP_POS[1][40]), BP_END[1] - 1})), _random_row(rs, 1, 4, 2)]]}
    # 3: both chromatids are the same list (every pair of positions identical by descent), mutations included
    twin0, twin1 = _random_row(rs, 0, 25, 12, cuts_extra=[E(CROWDED) + 100, E(CROWDED) + 40_000]), _random_row(rs, 1, 5, 3)
    twin = {"sex": 2, "chr": [[twin0, (list(twin0[0]), list(twin0[1]))], [twin1, (list(twin1[0]), list(twin1[1]))]]}
    # 4, 5: mosaics of the destination's own founders (short tracts shared with the residents), moderate lists
    def local(sex):
        chrs = []
        for k in range(NCHR):
            pair = []
            for h in range(2):
                parts, muts = _random_row(rs, k, 30 if k == 0 else 6, 8)
                pair.append(([(st, en, int(rs.randint(n_founders(0))), 0) for st, en, _, _ in parts], muts))
            chrs.append(pair)
        return {"sex": sex, "chr": chrs}
    first_record = [one, many, onedge, twin, local(1), local(2)]
    second_record = [{"sex": 2, "chr": [[_random_row(rs, k, 12, 5), _random_row(rs, k, 3, 0)] for k in range(NCHR)]},
                     {"sex": 1, "chr": [[_random_row(rs, k, 2, 40), _random_row(rs, k, 70 if k == 0 else 8, 1)] for k in range(NCHR)]}]
    return first_record, second_record


IMMIGRANTS, IMMIGRANTS_B = _build()


def rows_of(individuals, k):
    """the 2 n (parts, muts) of chromosome k in haplotype row order"""
    return [ind["chr"][k][h] for ind in individuals for h in range(2)]


def assert_coverage(individuals=None):
    """every property the issue names, on chromosome 0 of the first record"""
    rows = rows_of(IMMIGRANTS if individuals is None else individuals, 0)
    seg = lambda x: min(max(x - BP0[0], 0) >> LGW, N_RANGES - 1)
    assert N_RANGES == 31
    assert any(len(p) == 1 for p, _ in rows), "a one-part row"
    assert any(len(p) >= 300 for p, _ in rows), "a row of at least 300 parts"
    crowded = False
    for parts, _ in rows:
        per = np.bincount([seg(st) for st, _, _, _ in parts], minlength=N_RANGES)
        crowded |= any(per[t] >= 40 and per[t - 1] == 0 and per[t + 1] == 0 for t in range(1, N_RANGES - 1))
    assert crowded, "at least 40 parts in one range, none in its neighbours"
    starts = {st for parts, _ in rows for st, _, _, _ in parts}
    assert any({edge(t) - 1, edge(t), edge(t) + 1} <= starts for t in range(1, N_RANGES - 1)), "parts that start on a range edge and one bp to either side"
    assert {edge(N_RANGES - 1) - 1, edge(N_RANGES - 1), edge(N_RANGES - 1) + 1} <= starts, "the same at the last range"
    zero = {st for parts, _ in rows for st, en, _, _ in parts if st == en}
    assert any((z - BP0[0]) % (1 << LGW) == 0 and z < BP_END[0] for z in zero) and BP_END[0] in zero, "zero-length parts on a range edge and at the last map position"
    assert any(len(m) == 0 for _, m in rows) and any(len(m) >= 300 for _, m in rows), "a row without a mutation and one with at least 300"
    muts = {m for _, ms in rows for m in ms}
    cvs = {int(x) for p in range(NPHEN) for x in CV_POS[p][0]}
    assert any((m - BP0[0]) % (1 << LGW) == 0 and m > BP0[0] for m in muts), "a mutation on a range edge"
    assert any(m in {st for st, _, _, _ in parts[1:]} for parts, ms in rows for m in ms), "a mutation on a part boundary"
    assert muts & {int(x) for x in SNP_POS[0]} and muts & cvs and CV_PAIR_POS[0] in muts, "mutations on a SNP, on a CV and on the CV pair of equal positions"
    assert sum(int(x) == CV_PAIR_POS[0] for x in CV_POS[0][0]) == 2
    assert BP0[0] in muts and BP_END[0] - 1 in muts, "mutations on the first map position and on the last covered one"
    labels = {(hap, rp) for parts, _ in rows for _, _, hap, rp in parts}
    assert all((0, rp) in labels and (n_founders(rp) - 1, rp) in labels for rp in range(N_POP)), "hap_index 0 and the last founder of every root population"
    inds = IMMIGRANTS if individuals is None else individuals
    assert any(ind["chr"][0][0] == ind["chr"][0][1] and len(ind["chr"][0][0][0]) > 1 for ind in inds), "an individual whose chromatids are the same list"
    assert {ind["sex"] for ind in inds} == {1, 2}


assert_coverage()


# ---- the truth -------------------------------------------------------------------------------------------------------------------------
def _covering_part(parts, pos):
    for st, en, hap, rp in parts:
        if st <= pos < en:
            return hap, rp
    return None


def raster_rows(individuals, k, mutations=True):
    """genotype bits [2 n][L]: the founder bit under the part that covers the SNP's position, XOR membership in the row's mutation list
    (mutations=False: the row as the pool holds it)"""
    out = np.zeros((2 * len(individuals), LS[k]), dtype=np.uint8)
    for r, (parts, muts) in enumerate(rows_of(individuals, k)):
        mset = set(int(m) for m in muts) if mutations else set()
        for j, pos in enumerate(SNP_POS[k].tolist()):
            cov = _covering_part(parts, pos)
            if cov is not None:
                out[r, j] = FOUNDERS[k][cov[1]][cov[0]][j] ^ (pos in mset)
    return out


def raster_cv(individuals, p, k):
    """CV alleles [2 n][C] in file order: the CV founder bit under the covering part, flipped once if the position is in the mutation list"""
    out = np.zeros((2 * len(individuals), N_CV[p][k]), dtype=np.uint8)
    for r, (parts, muts) in enumerate(rows_of(individuals, k)):
        mset = set(int(m) for m in muts)
        for icv, pos in enumerate(CV_POS[p][k].tolist()):
            cov = _covering_part(parts, pos)
            if cov is not None:
                out[r, icv] = CV_FOUNDERS[p][k][cov[1]][cov[0]][icv] ^ (pos in mset)
    return out


def lists_as_downloaded(individuals, k):
    """(parts, part offsets, mutations, mutation offsets) as download_intervals / download_mutations return them for these rows alone"""
    rows = rows_of(individuals, k)
    flat = [q for parts, _ in rows for q in parts]
    parts = np.zeros(len(flat), dtype=PART_DTYPE)
    for col, name in enumerate(("st", "en", "hap_index", "root_population")):
        parts[name] = [q[col] for q in flat]
    poff = np.r_[0, np.cumsum([len(p) for p, _ in rows])].astype(np.uint64)
    muts = np.array([m for _, ms in rows for m in ms], dtype=np.uint64)
    moff = np.r_[0, np.cumsum([len(m) for _, m in rows])].astype(np.uint64)
    return parts, poff, muts, moff


def individuals_from_downloads(sex, parts_by_chr, muts_by_chr, who):
    """the individuals `who` of a population as this module's structure, from (parts, offsets) and (muts, offsets) per chromosome"""
    out = []
    for j, i in enumerate(who):
        chrs = []
        for (parts, poff), (muts, moff) in zip(parts_by_chr, muts_by_chr):
            pair = []
            for h in range(2):
                r = 2 * i + h
                q = parts[int(poff[r]):int(poff[r + 1])]
                pair.append(([(int(x["st"]), int(x["en"]), int(x["hap_index"]), int(x["root_population"])) for x in q], [int(m) for m in muts[int(moff[r]):int(moff[r + 1])]]))
            chrs.append(pair)
        out.append({"sex": int(sex[j]), "chr": chrs})
    return out


def encode(individuals, rows_travel, active=None, want_mask=False):
    """helpers.encode_record on this module's setting"""
    from tests import helpers
    return helpers.encode_record(individuals, LS, CV_POS, N_POP, rows_travel, active=active, founders=FOUNDERS, cv_founders=CV_FOUNDERS, snp_pos=SNP_POS,
                                 span=SPAN, want_mask=want_mask)


def apply_static(ctx, device, founder_rows=True, panels=False):
    """maps, SNPs, CVs and the uploaded founders of all three populations on a context of the library (device) or of the oracle"""
    for pop in range(N_POP):
        for k in range(NCHR):
            ctx.set_rmap(pop, k, RMAP_BP[k], RMAP_PROB[k], MAP_STEP[k]); ctx.set_mutmap(pop, k, RMAP_BP[k], MUT_RATE[k]); ctx.set_snps(pop, k, SNP_POS[k])
            words = pack_rows(FOUNDERS[k][pop])
            if founder_rows:
                ctx.upload_founders(pop, k, words, LS[k])
            if device and panels:
                ctx.upload_founder_panel(pop, k, words, LS[k])
            for p in range(NPHEN):
                ctx.set_cvs(pop, p, k, CV_POS[p][k], CV_A[pop][p][k], CV_D[pop][p][k], CV_VD)
                ctx.upload_cv_founders(pop, p, k, pack_rows(CV_FOUNDERS[p][k][pop]), N_CV[p][k])
