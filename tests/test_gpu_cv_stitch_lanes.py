"""The two forms of the CV-plane stitch: k_stitch_small (a half-wave per offspring row) and k_stitch_small8 (eight lanes per row,
four rounds per workgroup, one parental load where a lane's masks agree).  Every case runs three contexts side by
side on the same inputs -- the library with the old form forced, the library with the new form where it is legal, and the CPU
oracle -- for two generations, and compares after each: the resolved CV alleles of every phenotype (download_cv), A/D, the allele
frequencies and what the generation call hands back to the host from its status block (sexes, the redo count, the stitch totals).
The two library contexts must agree byte for byte, and both with the oracle.  Nothing has a tolerance.

Inputs (tests/ad_chain.py supplies the chromosome, the loci and the mutation map that aims new mutations at CV positions):
  * rows 2N = 2, 14, 130, 258, 770: a partial wave, a partial round, one workgroup and a row, a partial last workgroup of four;
  * C = 128, 1000, 1024 (4 / 32 / 32 words) take the new form; C = 96 (3 words: not whole 16-byte chunks) and C = 1500 (over 1024
    columns: 47 words, no fused counts) keep the old one, whatever the setter says;
  * MIXED: 40 map rows at 0.12 give gametes without a crossover, with one, and with 9 and more (the lanes' second search round)
    in the same generation, and a group of eight rows whose trip count is set by another row than the one without crossovers;
  * PLACED: a map of one-base-pair steps (bp_dist = 1: a breakpoint is its row's position) whose rows sit before the first CV, on
    a CV, one behind it, on both sides of the 32-bit edges 31|32 and 63|64, of the 128-bit edges 127|128 and 511|512, and behind the
    last CV;
  * two root populations: a second sub-row (root-population bits) blended by the same masks."""
import numpy as np
import pytest

from tests import ad_chain as ac
from tests import helpers

pytestmark = pytest.mark.gpu

OLD, NEW = 1, 2                                  # gev_set_cv_stitch_form
P0 = 20                                          # individuals of generation 0
CHAINS = [(7, 1), (65, 7), (129, 65), (385, 129), (7, 385)]      # offspring of generation 1, of generation 2


def cv_positions(ncv):
    pos = (1500 + 100 * np.arange(ncv)).astype(np.uint64)
    assert int(pos[-1]) < ac.BP_END
    return pos


def mixed_map(rate=0.12):
    return ac.RBP, np.r_[0.0, np.full(ac.R - 2, rate), 0.0], 5000


def placed_map(ncv, prob=0.3):
    """rows one base pair wide at chosen places of the CV grid of ncv columns: (bp, prob, 1), the columns the breakpoints fall on"""
    pos = cv_positions(ncv)
    ids = [0, 1, 2] + [e + d for e in (32, 64, 128, 512) if e + 1 < ncv for d in (-1, 0, 1)] + [ncv - 1, ncv]
    at = {1200: 0}                                                       # before the first CV
    for i in sorted(set(ids)):                                           # a breakpoint with exactly i columns in front of it
        x = int(pos[i - 1]) + 1 if i else 1300
        at[x] = i
        if i < ncv:
            at[int(pos[i])] = i                                          # ... and the one exactly ON column i: the same index
    at[int(pos[-1]) + 700] = ncv                                         # far behind the last CV
    xs = sorted(at)
    bp = np.array([ac.BP0] + xs + [ac.BP_END], dtype=np.uint64)
    return (bp, np.r_[0.0, np.full(len(xs), prob), 0.0], 1), [at[x] for x in xs]


class Plan:
    def __init__(self, ncv, rmap, n_pop=1):
        self.ncv = list(ncv); self.rmap, self.n_pop = rmap, n_pop        # one phenotype per entry of ncv
        rs = np.random.RandomState(3)
        self.cv = [(cv_positions(n), rs.randn(n), 0.3 * rs.randn(n), 0.0 if p == 0 else 0.5) for p, n in enumerate(self.ncv)]
        self.mmap = ac.mutation_map(ac.hot_positions(self.cv[0][0]))

    def context(self, lib, form=None):
        ctx = lib.create(self.n_pop, 1, len(self.ncv))
        if form is not None:
            ctx.set_cv_stitch_form(form)
        for pop in range(self.n_pop):
            ctx.set_rmap(pop, 0, *self.rmap)
            ctx.set_mutmap(pop, 0, self.mmap[0], self.mmap[1])
            ctx.set_snps(pop, 0, ac.SNPS)
            for p, cv in enumerate(self.cv):
                ctx.set_cvs(pop, p, 0, *cv)
        ctx.upload_founders(0, 0, ac.synth_packed(11, 2 * P0, ac.L), ac.L)
        for p, n in enumerate(self.ncv):
            ctx.upload_cv_founders(0, p, 0, ac.synth_packed(31 + 7 * p, 2 * P0, n), n)
        return ctx


def _generation(ctx, gen, n, n_parents):
    couples = np.array([(i % n_parents, (i + 1) % n_parents, 0, 1) for i in range(n)], dtype=np.int64)
    return ctx.reproduce(0, couples, 500 + gen, (1000 * gen + 17 * np.arange(n)).astype(np.uint32))


def _observed(ctx, plan, sex, device):
    out = {"sex": sex, "ad": ctx.compute_ad(0)}
    for p in range(len(plan.ncv)):
        out[f"cv {p}"] = ctx.download_cv(0, p, 0)
        out[f"frq {p}"] = ctx.get_cv_freq(0, p, 0).view(np.uint64)
    if device:
        out["redo"] = ctx.redo_count(); out["stitch"] = ctx.stitch_totals()
    return out


def _assert_same(a, b, label):
    for key in a:
        if key not in b:
            continue
        if key == "ad":
            for x, y in zip(a[key], b[key]):
                assert helpers.bits_equal(x, y), f"{label}: A/D"
        elif isinstance(a[key], np.ndarray):
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), f"{label}: {key}"
        else:
            assert a[key] == b[key], f"{label}: {key}"


def crossover_counts(o):
    """crossovers of every gamete of generation 1 (its parents' haplotypes are one part each, neighbours differ in hap_index)"""
    _, off = o.download_intervals(0, 0)
    return np.diff(off.astype(np.int64)) - 1


def _run(gpu_lib, oracle_lib, plan, chain, new_is_legal, label, new_form=NEW, after_first=None):
    g_old, g_new, o = plan.context(gpu_lib, OLD), plan.context(gpu_lib, new_form), plan.context(oracle_lib)
    ctxs = (g_old, g_new, o)
    sexes = [c.init_gen0(0, P0, 77) for c in ctxs]
    assert np.array_equal(sexes[0], sexes[2]) and np.array_equal(sexes[1], sexes[2])
    parents = P0
    for gen, n in enumerate(chain, 1):
        obs = [_observed(c, plan, _generation(c, gen, n, parents), c is not o) for c in ctxs]
        _assert_same(obs[0], obs[1], f"{label}, generation {gen}: old form against new form")
        _assert_same(obs[2], obs[0], f"{label}, generation {gen}: old form against the oracle")
        _assert_same(obs[2], obs[1], f"{label}, generation {gen}: new form against the oracle")
        lo, ln = g_old.dbg_cv_stitch_launches(), g_new.dbg_cv_stitch_launches()      # (a generation enqueued again launches again)
        assert lo[0] >= gen and lo[1] == 0, f"{label}: the old form was asked for, launches {lo}"
        assert (ln[1] >= gen and ln[0] == 0) if new_is_legal else (ln[0] >= gen and ln[1] == 0), f"{label}: generation {gen}, launches {ln}"
        if plan.n_pop == 1 and max(plan.ncv) <= 1024:
            assert g_new.dbg_ad_path() == ac.WIDE + ac.FROM_COUNTS, f"{label}: the fused column counts were not used"
        if gen == 1 and after_first:
            after_first(o)
        parents = n
    for c in ctxs:
        c.close()


def _mixed_claims(o):
    k = crossover_counts(o)
    assert (k == 0).any() and (k == 1).any() and 9 <= k.max() <= 40, sorted(set(k.tolist()))
    groups = k[:len(k) // 8 * 8].reshape(-1, 8)
    assert ((groups.max(axis=1) >= 9) & (groups.min(axis=1) <= 1)).any(), "no group of eight rows with k >= 9 beside k <= 1"


@pytest.mark.parametrize("chain", CHAINS, ids=lambda c: f"{2 * c[0]}-{2 * c[1]}rows")
@pytest.mark.parametrize("ncv", [128, 1000, 1024])
def test_new_form_equals_old_form_and_oracle(gpu_lib, oracle_lib, ncv, chain):
    claims = _mixed_claims if chain[0] == 385 else None
    _run(gpu_lib, oracle_lib, Plan([ncv], mixed_map()), chain, True, f"C = {ncv}, rows {chain}", after_first=claims)


@pytest.mark.parametrize("chain", [(129, 7), (7, 385)], ids=lambda c: f"{2 * c[0]}-{2 * c[1]}rows")
@pytest.mark.parametrize("ncv", [96, 1500])
def test_other_shapes_keep_the_old_form(gpu_lib, oracle_lib, ncv, chain):
    _run(gpu_lib, oracle_lib, Plan([ncv], mixed_map()), chain, False, f"C = {ncv}, rows {chain}")


def test_a_launch_with_one_unfit_plane_keeps_the_old_form(gpu_lib, oracle_lib):
    """two phenotypes = two work entries of one launch: 1000 columns would fit, 96 do not"""
    _run(gpu_lib, oracle_lib, Plan([1000, 96], mixed_map()), (129, 65), False, "C = 1000 and 96")


def test_two_fit_planes_of_different_length(gpu_lib, oracle_lib):
    _run(gpu_lib, oracle_lib, Plan([1000, 128], mixed_map()), (129, 65), True, "C = 1000 and 128")


def test_default_is_the_new_form_where_legal(gpu_lib, oracle_lib):
    _run(gpu_lib, oracle_lib, Plan([1000], mixed_map()), (65, 7), True, "automatic", new_form=None)


@pytest.mark.parametrize("rate", [0.01, 0.4])
def test_few_and_many_crossovers(gpu_lib, oracle_lib, rate):
    """0.01: most gametes without a crossover, some with one (one parental load per lane almost everywhere); 0.4: every gamete
    has more than eight (two or three search rounds for every row)"""
    def claims(o):
        k = crossover_counts(o)
        assert (k.max() <= 3 and (k == 0).sum() > len(k) // 2 and (k == 1).any()) if rate < 0.1 else (k.min() >= 5 and (k > 16).any() and k.max() <= 40), sorted(set(k.tolist()))
    _run(gpu_lib, oracle_lib, Plan([1000], mixed_map(rate)), (129, 65), True, f"rate {rate}", after_first=claims)


@pytest.mark.parametrize("ncv", [128, 1000, 1024])
def test_placed_breakpoints(gpu_lib, oracle_lib, ncv):
    rmap, ids = placed_map(ncv)
    assert {0, 1, 31, 32, 33, ncv - 1, ncv} <= set(ids) and (ncv == 128 or {127, 128, 129, 511, 512, 513} <= set(ids))

    def claims(o):                                                       # every placed row was hit by some gamete of generation 1
        parts, _ = o.download_intervals(0, 0)
        ends = set(int(x) for x in parts["en"])
        assert all(int(x) in ends for x in rmap[0][1:-1]), "a placed breakpoint that no gamete has"
    _run(gpu_lib, oracle_lib, Plan([ncv], rmap), (129, 65), True, f"placed, C = {ncv}", after_first=claims)


@pytest.mark.parametrize("ncv", [128, 1000])
def test_two_root_populations(gpu_lib, oracle_lib, ncv):
    """a second sub-row per plane row (nsub = 2): the rows are 8 / 64 words long"""
    _run(gpu_lib, oracle_lib, Plan([ncv], mixed_map(), n_pop=2), (129, 7), True, f"two root populations, C = {ncv}")


def test_setter_refuses_what_it_does_not_know(gpu_lib):
    from geneevolve_amd import capi
    ctx = gpu_lib.create(1, 1, 1)
    for bad in (-1, 3):
        with pytest.raises(capi.GevError):
            ctx.set_cv_stitch_form(bad)
    assert ctx.dbg_cv_stitch_launches() == (0, 0)
    ctx.close()
