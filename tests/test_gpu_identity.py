"""gev_identity_states: Jacquard's nine identity states per pair of individuals walked on the device from the ancestry interval lists,
against the table lookup of tests/identity_inputs.py on the lists gev_download_intervals returns and against the same header built for
the host: the inbred population of tests/test_gpu_ibd.py (every state in many pairs), individual ranges around the 16-tile and the
8-block of a wave with sub-blocks of 5, empty requests, a context without genotype planes, the exact integer identities that tie the
planes to gev_ibd_sharing, two populations behind a migration, the refusals (pytest -m gpu)."""
import numpy as np
import pytest

from geneevolve_amd import capi, identity
from geneevolve_amd.host import Simulation, SyntheticConfig
from tests import identity_inputs as J

pytestmark = pytest.mark.gpu

N, GENS = 40, 12                                        # the population of tests/test_gpu_ibd.py: 40 individuals, 12 generations, seed 4242
RANGES = [(0, 40), (1, 1), (3, 17), (7, 9), (15, 18), (32, 8), (39, 1)]
SIGMA = [0, 1, 4, 5, 2, 3, 6, 7, 8]                     # the plane of (b, a) that holds plane s of (a, b)


def inbred_config():
    return SyntheticConfig(N, 64, nchr=1, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.02, mut_per_row=2e-3, n_cv=8, seed=5)


def build_inbred(lib, dense=True):
    cfg = inbred_config()
    ctx = lib.create(1, 1, 1)
    if not dense:
        ctx.set_dense_state(False)
    cfg.apply_static(ctx)
    if dense:
        ctx.synth_founders(0, 0, 2 * N, 31)
    ctx.synth_cv_founders(0, 0, 0, 2 * N, 32)
    sim = Simulation(ctx, 4242, 1, True)
    sim.ras_initial_human_gen0(0, N)
    for _ in range(GENS):
        sim.next_generation_rm(0, N)
    return ctx


def fixture_conditions(parts, off, want, span):
    """what the cases below need of the population, asserted from the truth -> the pairs (i < k) with base pairs in each state"""
    for r in range(len(off) - 1):
        mine = parts[int(off[r]):int(off[r + 1])]
        assert sum(int(x["en"]) - int(x["st"]) for x in mine) == span, f"row {r} is not covered over the whole span"
    upper = np.triu(np.ones((N, N), dtype=bool), 1)
    pairs = [int((want[s][upper] > 0).sum()) for s in range(9)]
    assert upper.sum() == 780 and min(pairs) >= 8, f"pairs with base pairs in D1 .. D9: {pairs}"
    return pairs


class Inbred:
    def __init__(self, lib):
        self.lib = lib
        self.ctx = build_inbred(lib)
        self.parts, self.off = self.ctx.download_intervals(0, 0)
        self.span = int(inbred_config().rmap_bp[-1] - inbred_config().rmap_bp[0])
        self.want = J.truth(self.parts, self.off)              # computed once and left unchanged
        self.want.setflags(write=False)
        self.pairs = fixture_conditions(self.parts, self.off, self.want, self.span)


@pytest.fixture(scope="module")
def inbred(gpu_lib):
    fx = Inbred(gpu_lib)
    print("inbred: pairs of 780 with base pairs in D1 .. D9:", fx.pairs)
    yield fx
    fx.ctx.close()


def same(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, f"{what}: {got.dtype}{got.shape}, expected uint64{want.shape}"
    assert np.array_equal(got, want), f"{what}: differs at {np.argwhere(got != want)[:5].tolist()}"


def test_all_individuals_against_all(inbred):
    """device == truth == host build; a repeat gives the same bytes; identity.states over the one chromosome is the call"""
    got = inbred.ctx.identity_states(0, 0)
    same(got, inbred.want, "device against the truth")
    same(inbred.lib.dbg_identity_host(inbred.parts, inbred.off), inbred.want, "host build against the truth")
    again = inbred.ctx.identity_states(0, 0)
    assert again.tobytes() == got.tobytes(), "the call repeated"
    same(identity.states(inbred.ctx, 0), inbred.want, "identity.states")
    same(identity.states(inbred.ctx, 0, ind=(3, 17), ind_b=range(15, 33)), inbred.want[:, 3:20, 15:33], "identity.states, a block")


@pytest.mark.parametrize("a0,na", RANGES)
def test_ranges_around_the_tile_and_the_wave_block(inbred, a0, na):
    """the A range against every B range in sub-blocks of 5 individuals a side, whose edges fall inside tiles and wave blocks"""
    ctx = inbred.ctx
    ctx.dbg_output_chunk(5)
    try:
        for b0, nb in RANGES:
            same(ctx.identity_states(0, 0, a0, na, 0, b0, nb), inbred.want[:, a0:a0 + na, b0:b0 + nb], f"individuals [{a0},+{na}) x [{b0},+{nb}), sub-blocks of 5")
    finally:
        ctx.dbg_output_chunk(0)
    same(ctx.identity_states(0, 0, a0, na), inbred.want[:, a0:a0 + na, :], f"individuals [{a0},+{na}) x all, one sub-block")


def test_empty_requests(inbred):
    ctx = inbred.ctx
    bp = np.full((9, 3, 4), 7, dtype=np.uint64)
    for na, nb in ((0, 4), (3, 0), (0, 0)):
        ctx._call("identity_states", 0, 0, 5, na, 0, 9, nb, bp)
        assert (bp == 7).all()
    ctx._call("identity_states", 0, 0, N, 0, 0, 0, 4, None)          # an empty range at the end, no buffer
    assert ctx.identity_states(0, 0, 5, 0).shape == (9, 0, N)


def test_integer_identities_with_ibd_sharing(inbred):
    """exact, against ctx.ibd_sharing at min_bp 0: the planes sum to the span; 4 D1 + 2 (D3 + D5 + D7) + D8 is the four haplotype pairs'
    shared length; D1 + D2 + D3 + D4 is a's own shared length for every b, and likewise for b; the diagonal; the transpose"""
    D = inbred.ctx.identity_states(0, 0).astype(np.int64)
    sh = inbred.ctx.ibd_sharing(0, 0, want=(True, False, False))[0].astype(np.int64)
    assert (D.sum(axis=0) == inbred.span).all()
    four = sh[0::2, 0::2] + sh[0::2, 1::2] + sh[1::2, 0::2] + sh[1::2, 1::2]
    assert np.array_equal(4 * D[0] + 2 * (D[2] + D[4] + D[6]) + D[7], four)
    own = sh[np.arange(0, 2 * N, 2), np.arange(1, 2 * N, 2)]
    assert np.array_equal(D[0] + D[1] + D[2] + D[3], np.repeat(own[:, None], N, axis=1))
    assert np.array_equal(D[0] + D[1] + D[4] + D[5], np.repeat(own[None, :], N, axis=0))
    for i in range(N):
        assert D[:, i, i].tolist() == [own[i], 0, 0, 0, 0, 0, inbred.span - own[i], 0, 0], i
    assert (own > 0).any(), "twelve generations of 40 were meant to leave inbred individuals"
    for s in range(9):
        assert np.array_equal(D[s], D[SIGMA[s]].T), s


def test_statistics(inbred):
    """identity.py on the device's planes against the module-free arithmetic of the truth, pair by pair"""
    from fractions import Fraction
    D = identity.states(inbred.ctx, 0)
    kin, (k0, k1, k2), (fa, fb), jac = identity.kinship(D), identity.ibd012(D), identity.inbreeding(D), identity.jacquard(D)
    for i in range(0, N, 3):
        for k in range(N):
            w = J.fractions_of(inbred.want, i, k)
            for g, x in ((kin[i, k], w["kinship"]), (k0[i, k], w["k0"]), (k1[i, k], w["k1"]), (k2[i, k], w["k2"]), (fa[i, k], w["f_a"]), (fb[i, k], w["f_b"]), (jac[8, i, k], w["jacquard"][8])):
                assert abs(Fraction(float(g)) - x) <= x * Fraction(1, 10 ** 15), (i, k)
    assert np.array_equal(identity.fraternity(D), k2)


def test_plane_less_context(gpu_lib):
    """the same run without genotype planes: equal to the truth of its own lists"""
    ctx = build_inbred(gpu_lib, dense=False)
    parts, off = ctx.download_intervals(0, 0)
    want = J.truth(parts, off)
    fixture_conditions(parts, off, want, int(inbred_config().rmap_bp[-1] - inbred_config().rmap_bp[0]))
    same(ctx.identity_states(0, 0), want, "plane-less context")
    same(ctx.identity_states(0, 0, 3, 17, 0, 15, 18), want[:, 3:20, 15:33], "plane-less context, a block")
    ctx.close()


def test_two_populations_behind_a_migration(gpu_lib):
    """populations of 12 and 9 on two chromosomes: two generations, three individuals move from population 0 to 1 and the first call
    comes directly behind the move (it materialises the pending order), three more generations of population 1"""
    from tests.test_gpu_migrant_record import SIZES, scenario
    g, sim, _, _ = scenario(gpu_lib, True, True)
    sim.ras_do_migration([(0, 7, 1), (0, 4, 1), (0, 0, 1)])
    first = [g.identity_states(k, 0, pop_b=1) for k in range(2)]
    assert g.pop_size(0) == SIZES[0] - 3 and g.pop_size(1) == SIZES[1] + 3
    for k in range(2):
        pa, oa = g.download_intervals(0, k); pb, ob = g.download_intervals(1, k)
        assert first[k].shape == (9, SIZES[0] - 3, SIZES[1] + 3)
        same(first[k], J.truth(pa, oa, pb, ob), f"directly behind the migration, chromosome {k}")
    for _ in range(3):
        sim.next_generation_rm(1, SIZES[1] + 3)
    total = np.zeros((9, SIZES[0] - 3, SIZES[1] + 3), dtype=np.uint64)
    for k in range(2):
        pa, oa = g.download_intervals(0, k); pb, ob = g.download_intervals(1, k)
        want = J.truth(pa, oa, pb, ob)
        same(g.identity_states(k, 0, pop_b=1), want, f"population 0 x population 1, chromosome {k}")
        same(g.identity_states(k, 1, 1, 8, 0, 2, 5), J.transposed(want)[:, 1:9, 2:7], f"population 1 x population 0, a block, chromosome {k}")
        same(gpu_lib.dbg_identity_host(pa, oa, pb, ob), want, f"host build, chromosome {k}")
        total += want
    same(identity.states(g, 0, pop_b=1), total, "identity.states over both chromosomes")
    assert (total.sum(axis=0) == sum(g._span_bp[(1, k)] for k in range(2))).all()
    assert (total[[0, 2, 4, 6, 7]].sum(axis=0) > 0).any(), "the populations were meant to share founders behind the migration"
    g.close()


def test_refusals(gpu_lib):
    """each gives the documented code and message and leaves the output untouched; GEV_ESTATE as gev_ibd_sharing gives it"""
    bp = np.full((9, 2, 2), 7, dtype=np.uint64)
    sh = np.full((2, 2), 7, dtype=np.uint64)

    def refused(ctx, code, a=(0, 2), b=(0, 2), chr=0, message=None, out=bp):
        rc = ctx.L._f("identity_states")(ctx.h, chr, 0, a[0], a[1], 0, b[0], b[1], out)
        mine = ctx.L.last_error()
        assert rc == code and (bp == 7).all(), f"{rc} {mine}"
        if message is None:                                         # the words of gev_ibd_sharing on the same context, under this call's name
            assert ctx.L._f("ibd_sharing")(ctx.h, chr, 0, 0, 2, 0, 0, 2, 0, sh, None, None) == code and (sh == 7).all()
            message = ctx.L.last_error().replace("ibd_sharing", "identity_states")
        assert mine == message, mine

    off = build_inbred(gpu_lib)
    off.set_track_intervals(False)
    refused(off, -2)
    assert "interval tracking is disabled" in off.L.last_error()
    off.close()
    cfg = SyntheticConfig(N, 64, nchr=2, chrom_bp=2_000_000, map_step=20_000, rec_per_row=0.02, mut_per_row=2e-3, n_cv=8, seed=5)
    two = gpu_lib.create(1, 2, 1)
    for c in range(2):
        two.set_rmap(0, c, cfg.rmap_bp, cfg.rmap_prob, cfg.bp_dist); two.set_mutmap(0, c, cfg.mut_bp, cfg.mut_rate)
    two.set_snps(0, 0, cfg.snp_pos)
    two.set_cvs(0, 0, 0, *cfg.cv[0][0], cfg.vd)
    two.set_chr_active(1, False)
    two.synth_founders(0, 0, 2 * N, 31); two.synth_cv_founders(0, 0, 0, 2 * N, 32)
    refused(two, -2)
    assert "no current generation" in two.L.last_error()
    two.init_gen0(0, N, 77)
    refused(two, -2, chr=1)
    assert "not active" in two.L.last_error()
    refused(two, -1, a=(N - 1, 2), message=f"identity_states: individuals (a) [{N - 1},{N + 1}) beyond the {N} there are")
    refused(two, -1, a=(N + 1, 0), message=f"identity_states: individuals (a) [{N + 1},{N + 1}) beyond the {N} there are")
    refused(two, -1, b=(N - 1, 2), message=f"identity_states: individuals (b) [{N - 1},{N + 1}) beyond the {N} there are")
    one = np.zeros(3, dtype=np.uint64)                               # the host form on an individual without parts, and no buffer
    assert gpu_lib._f("dbg_identity_host")(None, one, 1, None, one, 1, None) == -1
    host_words = gpu_lib.last_error()
    assert host_words == "dbg_identity_host: bp is null"
    refused(two, -1, out=None, message=host_words.replace("dbg_identity_host", "identity_states"))
    two.generation_begin(0, 12345, N)
    try:
        refused(two, -2)
        assert "pending" in two.L.last_error()
    finally:
        two.generation_end()
    assert two.identity_states(0, 0).shape == (9, N, N)
    two.close()
