"""Inputs built so that a crossover or a new mutation lands exactly where the case says (pure Python plus the oracle's kat_*
helpers; no GPU, no sampling code of the library or the oracle).

Random seeds on uniform maps reach the interesting places of the sampling kernels with probability near zero: the low digit of
generate_canonical decides about twice in 2^31 draws, no map in the suite has prob[0] > 0, and a hit on one particular draw index
is a matter of luck.  Here the map row under a chosen draw is given the probability that sits one ulp on either side of the draw's
own value, so the outcome hangs on the last bit of the comparison `r < p`.

Arithmetic (each line is pinned against the oracle by tests/test_placed_hits_cpu.py), M = 2^31 - 1:
  * an engine seeded with the unsigned expression E starts at s0 = E mod M (0 -> 1);
  * draw d uses outputs x1 = 16807^(2d+1) s0 (low digit) and x2 = 16807^(2d+2) s0 (high digit): a = x2 - 1, b = x1 - 1,
    r = kat_canonical(x1, x2);
  * the crossover scan of a gamete with seed s uses engine s + 1, draw d tests map row d (d = 0 .. R-1);
  * the mutation scan of a task with seed S uses engine S + 2, draw d tests map row d + 1 (d = 0 .. M-2); hit h takes output h + 1
    of engine S + 1 for its position and rand() output h of srand(S) for its side;
  * seed chain of Simulation::reproduce as restated in predict().

A Scenario holds every input of one generation from generation 0 and, after predict(), the record of every (offspring,
chromosome) task worked out from kat_rand / kat_uint / kat_canonical alone.  The DESIGNATED tasks are those a constructor placed a
draw for; constructors assert the placed outcome (hit / miss / count) on the prediction, so a Scenario that exists satisfies its
claim."""
import ctypes as C

import numpy as np

from oracle import oracle_api

M31 = 2147483647
G = 16807
NMAX = 2147483646
INV_G = pow(G, -1, M31)
SEARCH_BOUND = int(2e-3 * 2 ** 31)          # search_seed: a trial succeeds with probability 2e-3
SEARCH_CAP = 50_000                         # failure odds e^-100; reaching it is an error
search_trials = []                          # trial count of every search_seed call (the CPU test asserts the cap)

_MAXD = 4300
_POW_HI = np.array([pow(G, 2 * d + 2, M31) for d in range(_MAXD)], dtype=np.uint64)


# ---- engines and digits ---------------------------------------------------------------------
def engine_s0(E):
    x = (int(E) & 0xFFFFFFFF) % M31
    return x or 1


def digits(E, d):
    """(a, b) = (high, low) digit of draw d of minstd_rand0(E)"""
    x1 = pow(G, 2 * d + 1, M31) * engine_s0(E) % M31
    x2 = x1 * G % M31
    return x2 - 1, x1 - 1


def canonical(ol, a, b):
    return oracle_api.kat_canonical(ol, b + 1, a + 1)


def draw_value(ol, E, d):
    a, b = digits(E, d)
    return canonical(ol, a, b)


def high_digits(E, n):
    """a of draws 0 .. n-1 of minstd_rand0(E)"""
    return (_POW_HI[:n] * np.uint64(engine_s0(E))) % np.uint64(M31) - np.uint64(1)


def scan(ol, E, first_row, prob, n_draws):
    """rows hit by the Bernoulli scan `r < prob[first_row + d]`, d = 0 .. n_draws-1, on minstd_rand0(E).  r lies in
    [a / R, (a + 1) / R) up to rounding, R = 2^31 - 2, so only draws with a <= p R + 2 can hit: those are decided by kat_canonical"""
    if n_draws <= 0:
        return []
    a = high_digits(E, n_draws)
    p = np.asarray(prob[first_row:first_row + n_draws], dtype=np.float64)
    cand = np.flatnonzero((p > 0) & (a.astype(np.float64) <= p * float(NMAX) + 2.0))
    hits = []
    for d in cand:
        ad = int(a[d]); b = (ad + 1) * INV_G % M31 - 1
        if canonical(ol, ad, b) < p[d]:
            hits.append(first_row + int(d))
    return hits


# ---- primitives -------------------------------------------------------------------------------
def solve_seed(d, a, offset, wrap=False):
    """the seed whose engine `seed + offset` has high digit a on draw d (closed form).  wrap: the seed >= 2^31 with the same
    engine (exercises the signed Schrage step of srand)"""
    s0 = (a + 1) * pow(pow(G, 2 * d + 2, M31), -1, M31) % M31
    seed = s0 - offset
    if wrap or seed < 0:
        seed += M31
    assert 0 <= seed < 2 ** 32 and digits(seed + offset, d)[0] == a
    return seed


def search_seed(start, produced, d, bound=SEARCH_BOUND):
    """a gamete seed inside gev_reproduce is a rand() output and cannot be chosen: step the seed that produces it from `start`
    until draw d of the gamete's crossover scan has a < bound.  produced(S) = the gamete seed that producer seed S leads to"""
    for trial in range(1, SEARCH_CAP + 1):
        S = start + trial - 1
        if digits(produced(S) + 1, d)[0] < bound:
            search_trials.append(trial)
            return S
    raise RuntimeError(f"search_seed: no seed within {SEARCH_CAP} trials (d = {d})")


def straddle(r):
    """(p_hit, p_miss): the reference tests r < p"""
    return float(np.nextafter(r, 1.0)), float(r)


def fit_map_to_stream(ol, E, first_row, n_rows_total, n_draws, k):
    """probabilities for a map of n_rows_total rows: the k rows where the stream of engine E has its smallest high digits get the
    p_hit of their own draw, every other row 0; that scan then has exactly k hits and amax stays small"""
    a = high_digits(E, n_draws)
    ds = np.argsort(a, kind="stable")[:k]
    prob = np.zeros(n_rows_total)
    for d in ds:
        prob[first_row + int(d)] = straddle(draw_value(ol, E, int(d)))[0]
    return prob


def threshold(gl, p):
    """(a_lo, a_hi, b0, b1) of the library's integer threshold of probability p (host code)"""
    out = (C.c_uint32 * 4)()
    assert gl._f("dbg_threshold")(p, out) == 0
    return tuple(int(x) for x in out)


# ---- one generation, restated -------------------------------------------------------------------
def recombine(hap, start, locs):
    """Simulation::recombine for parts given as (st, en, hap_index) lists: hap = (Hap[0], Hap[1])"""
    h = start
    if len(locs) < 3:
        return list(hap[h])
    ret = []
    for i1 in range(1, len(locs)):
        H = hap[h]; L, Rr = locs[i1 - 1], locs[i1]
        i2 = 0
        while len(H) > i2 and H[i2][1] <= L:
            i2 += 1
        if len(H) > i2 and H[i2][0] < L < H[i2][1] and Rr < H[i2][1]:
            ret.append((L, Rr, H[i2][2])); i2 += 1
        if len(H) > i2 and H[i2][0] < L < H[i2][1] and Rr >= H[i2][1]:
            ret.append((L, H[i2][1], H[i2][2])); i2 += 1
        while len(H) > i2 and H[i2][1] <= Rr and L <= H[i2][0]:
            ret.append(H[i2]); i2 += 1
        if len(H) > i2 and H[i2][0] < Rr < H[i2][1]:
            ret.append((H[i2][0], Rr, H[i2][2]))
        h = (h + 1) % 2
    return ret


def predict_gamete(ol, rmap, seed):
    """one ras_sim_loc_rec call restated: (rows hit, breakpoints, the two rand() outputs behind the call)"""
    bp, prob, dist = rmap
    rows = scan(ol, seed + 1, 0, prob, len(bp))
    r = oracle_api.kat_rand(ol, seed, len(rows) + 2)
    return rows, [int(bp[row]) + int(r[i]) % int(dist) for i, row in enumerate(rows)], [int(r[len(rows)]), int(r[len(rows) + 1])]


class Scenario:
    """inputs of one generation from generation 0 (couples of one offspring each) and, after predict(), its expected outcome"""

    def __init__(self, name, n_ind, rmaps, mmaps, seed_reproduce, mut_seeds, seed_gen0=77):
        self.name, self.n_ind, self.nchr = name, n_ind, len(rmaps)
        self.rmaps = rmaps                  # per chromosome: (bp, prob, bp_dist)
        self.mmaps = mmaps                  # per chromosome: (bp, rate), or None: no mutation map (serial chain mode)
        self.seed_reproduce = int(seed_reproduce)
        self.mut_seeds = None if mmaps is None else np.asarray(mut_seeds, dtype=np.uint32)
        self.seed_gen0 = seed_gen0
        self.designated = []                # (task, what, note): what in {"pat", "mat", "mut"}
        self.claims = []                    # (task, what, kind, value): "hit" / "miss" row, "count" value
        self.tasks = None

    @property
    def n_tasks(self):
        return self.n_ind * self.nchr

    def without_mutation(self, name):
        """the same couples, maps and reproduce seed without a mutation map: task 0's gametes are the same, every later gamete
        chains through the crossover counts"""
        s = Scenario(name, self.n_ind, self.rmaps, None, self.seed_reproduce, None, self.seed_gen0)
        s.designated = [x for x in self.designated if x[0] == 0 and x[1] != "mut"]
        s.claims = [x for x in self.claims if x[0] == 0 and x[1] != "mut"]
        return s

    # -- the restatement: every record from kat_rand / kat_uint / kat_canonical
    def gamete(self, ol, c, seed, n_after):
        bp, prob, dist = self.rmaps[c]
        rows = scan(ol, seed + 1, 0, prob, len(bp))
        r = oracle_api.kat_rand(ol, seed, len(rows) + n_after)
        bks = [int(bp[row]) + int(r[i]) % int(dist) for i, row in enumerate(rows)]
        return dict(seed=int(seed), rows=rows, bks=bks, start=int(r[len(rows)]) % 2, after=[int(x) for x in r[len(rows) + 1:]])

    def mutations(self, ol, c, S, last):
        bp, rate = self.mmaps[c]
        rows = scan(ol, S + 2, 1, rate, len(bp) - 1)
        n = len(rows)
        r = oracle_api.kat_rand(ol, S, n + 2)
        pos = []
        for h, row in enumerate(rows):      # all ranges of a map are equally wide here: output h + 1 is hit h's, rejections included
            pos.append(int(oracle_api.kat_uint(ol, S + 1, int(bp[row - 1]), int(bp[row]), h + 1)[h]))
        return dict(seed=int(S), rows=rows, pos=pos, side=[int(r[h]) % 2 for h in range(n)],
                    sex=(int(r[n]) % 2 + 1) if last else None, next=int(r[n + 1] if last else r[n]))

    def predict(self, ol):
        while True:                         # the first generation-0 seed that gives both sexes
            sex0 = oracle_api.kat_rand(ol, self.seed_gen0, self.n_ind) % 2 + 1
            males, females = np.flatnonzero(sex0 == 1), np.flatnonzero(sex0 == 2)
            if len(males) and len(females):
                break
            self.seed_gen0 += 1
        self.sex0 = sex0.astype(np.uint8)
        self.couples = np.zeros((self.n_ind, 4), dtype=np.int64)
        for i in range(self.n_ind):
            self.couples[i] = (males[i % len(males)], females[(3 * i + 1) % len(females)], 0, 1)
        self.tasks, self.sex = [], np.zeros(self.n_ind, dtype=np.uint8)
        sp = int(oracle_api.kat_rand(ol, self.seed_reproduce, 1)[0])
        for t in range(self.n_tasks):
            c, last = t % self.nchr, t % self.nchr == self.nchr - 1
            pat = self.gamete(ol, c, sp, 2)
            mat = self.gamete(ol, c, pat["after"][0], 3)
            rec = dict(t=t, chr=c, ind=t // self.nchr, pat=pat, mat=mat, mut=None)
            if self.mmaps is not None:
                mu = rec["mut"] = self.mutations(ol, c, int(self.mut_seeds[t]), last)
                sex, sp = mu["sex"], mu["next"]
            else:
                sex, sp = (mat["after"][0] % 2 + 1, mat["after"][1]) if last else (None, mat["after"][0])
            if last:
                self.sex[t // self.nchr] = sex
            self.tasks.append(rec)
        for t, what, kind, value in self.claims:
            rows = self.tasks[t][what]["rows"]
            ok = {"hit": value in rows, "miss": value not in rows, "count": len(rows) == value}[kind]
            assert ok, f"{self.name}: task {t} {what}: placed {kind} {value} does not hold, rows {rows}"
        return self

    def expected_rows(self, t):
        """what the designated task's records make of generation 0: {row: (parts [(st, en, hap_index)], new mutations in list order)}"""
        rec = self.tasks[t]
        c, i = rec["chr"], rec["ind"]
        bp = self.rmaps[c][0]
        bp0, bp_end = int(bp[0]), int(bp[-1])
        out = {}
        for side, what, parent in ((0, "pat", self.couples[i][0]), (1, "mat", self.couples[i][1])):
            hap = ([(bp0, bp_end, 2 * int(parent))], [(bp0, bp_end, 2 * int(parent) + 1)])
            parts = recombine(hap, rec[what]["start"], [bp0] + rec[what]["bks"] + [bp_end])
            muts = []
            if rec["mut"] is not None:
                mine = [p for p, s in zip(rec["mut"]["pos"], rec["mut"]["side"]) if s == side]
                for st, en, _ in parts:
                    muts += [p for p in mine if st <= p < en]
            out[2 * i + side] = (parts, muts)
        return out

    # -- the inputs that do not bear on sampling: loci and causal variants around every placed event
    def static_inputs(self):
        rs = np.random.RandomState(4)
        snps, cvs = [], []
        for c in range(self.nchr):
            bp = self.rmaps[c][0]
            bp0, bp_end = int(bp[0]), int(bp[-1])
            near = []
            for t, what, _ in self.designated:
                rec = self.tasks[t]
                if rec["chr"] != c:
                    continue
                if what == "mut":
                    near += rec["mut"]["pos"]
                else:
                    for v in rec[what]["bks"]:
                        near += [v - 1, v]      # a locus on either side of the breakpoint
            near = sorted({v for v in near if bp0 <= v < bp_end})[:90]
            grid = np.linspace(bp0, bp_end - 1, 200).astype(np.int64)
            pos = np.unique(np.r_[grid, np.array(near, dtype=np.int64)]).astype(np.uint64)
            assert len(pos) <= 300
            snps.append(pos)
            cvp = np.unique(np.r_[np.array(near[:10], dtype=np.int64), grid[::10]])[:20].astype(np.uint64)
            cvs.append((cvp, rs.randn(len(cvp)), 0.3 * rs.randn(len(cvp))))
        return snps, cvs

    def apply(self, ctx, synth_packed=None):
        """static inputs, founders (synth_packed given: uploaded, the oracle's way; else generated on the device) and generation 0"""
        snps, cvs = self.static_inputs()
        nh = 2 * self.n_ind
        for c in range(self.nchr):
            bp, prob, dist = self.rmaps[c]
            ctx.set_rmap(0, c, bp, prob, dist)
            if self.mmaps is not None:
                ctx.set_mutmap(0, c, *self.mmaps[c])
            ctx.set_snps(0, c, snps[c])
            ctx.set_cvs(0, 0, c, cvs[c][0], cvs[c][1], cvs[c][2], 0.2)
        for c in range(self.nchr):
            if synth_packed is None:
                ctx.synth_founders(0, c, nh, 11 + c); ctx.synth_cv_founders(0, 0, c, nh, 31 + c)
            else:
                ctx.upload_founders(0, c, synth_packed(11 + c, nh, len(snps[c])), len(snps[c]))
                ctx.upload_cv_founders(0, 0, c, synth_packed(31 + c, nh, len(cvs[c][0])), len(cvs[c][0]))
        sex = ctx.init_gen0(0, self.n_ind, self.seed_gen0)
        assert np.array_equal(sex, self.sex0)

    def reproduce(self, ctx):
        return ctx.reproduce(0, self.couples, self.seed_reproduce, self.mut_seeds)

    def check_designated(self, ctx, label):
        """the stated expectation on every designated task, read from the lists of generation 1"""
        assert self.designated
        for t in sorted({t for t, _, _ in self.designated}):
            c = self.tasks[t]["chr"]
            parts, poff = ctx.download_intervals(0, c)
            muts, moff = ctx.download_mutations(0, c)
            for row, (want_parts, want_muts) in self.expected_rows(t).items():
                got = [(int(p["st"]), int(p["en"]), int(p["hap_index"])) for p in parts[int(poff[row]):int(poff[row + 1])]]
                assert got == want_parts, f"{label} {self.name}: task {t} row {row}: parts {got}, stated {want_parts}"
                assert all(int(p["root_population"]) == 0 for p in parts[int(poff[row]):int(poff[row + 1])])
                gm = [int(x) for x in muts[int(moff[row]):int(moff[row + 1])]]
                assert gm == want_muts, f"{label} {self.name}: task {t} row {row}: new mutations {gm}, stated {want_muts}"


# ---- maps ---------------------------------------------------------------------------------------
STEP = 1000


def rmap_rows(R, background=0.0):
    bp = (1000 + STEP * np.arange(R)).astype(np.uint64)
    return bp, np.full(R, float(background)), STEP


def mmap_rows(M, bp_end, background=0.0):
    """M rows of equal width inside [1000, bp_end): every new mutation lands inside the chromosome"""
    w = (bp_end - 1 - 1000) // (M - 1)
    assert w >= 1
    bp = (1000 + w * np.arange(M)).astype(np.uint64)
    rate = np.full(M, float(background)); rate[0] = 0.0
    return bp, rate


def edge_draws(n):
    """where family A places a hit in a scan of n draws"""
    ds = {0, n - 1}
    for lo, hi, need in ((63, 64, 65), (255, 256, 257), (2047, 2048, 2049)):
        if n >= need:
            ds |= {lo, hi}
    return sorted(ds)


N_DRAWS = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]
WARM = 5e-4


def _producer(ol, sc_mmaps, nchr, t_prev):
    """seed_pat[t_prev + 1] as a function of task t_prev's mutation seed (t_prev = -1: of the reproduce seed)"""
    if t_prev < 0:
        return lambda S: int(oracle_api.kat_rand(ol, S, 1)[0])
    c, last = t_prev % nchr, t_prev % nchr == nchr - 1
    bp, rate = sc_mmaps[c]

    def f(S):
        n = len(scan(ol, S + 2, 1, rate, len(bp) - 1))
        return int(oracle_api.kat_rand(ol, S, n + 2)[n + (1 if last else 0)])
    return f


def _place(ol, prob, row, E, d, hit):
    """give map row `row` the probability one ulp on the hit / miss side of draw d of engine E; returns that probability"""
    p_hit, p_miss = straddle(draw_value(ol, E, d))
    prob[row] = p_hit if hit else p_miss
    return prob[row]


def _a_target(i):
    return 1_500_000 + 104_729 * i          # high digits around 7e-4 .. 1.2e-3 of the range, all different


# ---- family A: draw-index edges, both scans, one scenario per (n, hit / miss, cold / warm) --------------
def family_a(ol, n, hit, warm):
    """reproduce form (has a mutation map): crossover hits at every edge draw of a map of R = n rows (one gamete per edge: the
    paternal gamete of tasks 0, 1, ..), mutation hits at every edge draw of a map of M = n + 1 rows (tasks behind them, seeds in
    closed form, every second one >= 2^31).  n = 1: mutation scan only, the smallest recombination map beside it"""
    bg = WARM if warm else 0.0
    R = max(n, 2)
    bp, rprob, dist = rmap_rows(R, bg if n >= 2 else 0.0)
    mbp, mrate = mmap_rows(n + 1, int(bp[-1]), bg)
    ds = edge_draws(n)
    n_x = len(ds) if n >= 2 else 0
    n_ind = max(n_x + len(ds) + 1, 3)
    # the mutation tasks first (closed form); their rows are part of the map the producers' own scans run on
    mut_seeds = np.array([1000 + 17 * t for t in range(n_ind)], dtype=np.int64)
    placed = []
    for i, d in enumerate(ds):
        t = n_x + i
        mut_seeds[t] = solve_seed(d, _a_target(i), 2, wrap=bool(i & 1))
        p = _place(ol, mrate, d + 1, int(mut_seeds[t]) + 2, d, hit)
        placed.append((t, "mut", d + 1, p, _a_target(i)))
    seed_reproduce = 4242
    for i, d in enumerate(ds[:n_x]):
        prod = _producer(ol, [(mbp, mrate)], 1, i - 1)
        if i == 0:
            seed_reproduce = S = search_seed(4242, prod, d)
        else:
            mut_seeds[i - 1] = S = search_seed(20_000 * i, prod, d)
        sp = prod(S)
        p = _place(ol, rprob, d, sp + 1, d, hit)
        placed.append((i, "pat", d, p, digits(sp + 1, d)[0]))
    sc = Scenario(f"A n={n} {'hit' if hit else 'miss'} {'warm' if warm else 'cold'}", n_ind, [(bp, rprob, dist)], [(mbp, mrate)], seed_reproduce, mut_seeds)
    for t, what, row, p, a in placed:
        sc.designated.append((t, what, f"row {row}"))
        sc.claims.append((t, what, "hit" if hit else "miss", row))
    sc.windows = [(p, a) for _, _, _, p, a in placed]
    return sc.predict(ol)


def family_a_task0(ol, n, d, hit, warm):
    """one crossover edge in the paternal gamete of task 0 (reproduce seed searched); the serial chain kernels take these"""
    bp, rprob, dist = rmap_rows(n, WARM if warm else 0.0)
    prod = _producer(ol, None, 1, -1)
    seed = search_seed(7000 + 13 * d, prod, d)
    sp = prod(seed)
    p = _place(ol, rprob, d, sp + 1, d, hit)
    sc = Scenario(f"A0 n={n} d={d} {'hit' if hit else 'miss'} {'warm' if warm else 'cold'}", 3, [(bp, rprob, dist)], None, seed, None)
    sc.designated.append((0, "pat", f"row {d}"))
    sc.claims.append((0, "pat", "hit" if hit else "miss", d))
    sc.windows = [(p, digits(sp + 1, d)[0])]
    return sc.predict(ol)


def gamete_cases_a(ol, n, hit, warm):
    """gev_dbg_sim_loc_rec form: (map, [(seed, row)]) with every edge of a map of n rows placed in closed form"""
    bp, rprob, dist = rmap_rows(n, WARM if warm else 0.0)
    seeds, windows = [], []
    for i, d in enumerate(edge_draws(n)):
        s = solve_seed(d, _a_target(i), 1, wrap=bool(i & 1))
        p = _place(ol, rprob, d, s + 1, d, hit)
        seeds.append((s, d)); windows.append((p, _a_target(i)))
    return (bp, rprob, dist), seeds, windows


# ---- family B: the second digit of the window (b1) ----------------------------------------------------
def b1_list(ol, n=400):
    """the fixed list of probabilities family B walks.  A window is two high digits wide only where generate_canonical is not
    monotone across a digit boundary: a R does not fit a double from a = 2^22 on, and where fl(a R) rounds up,
    canonical(a, R - 1) can exceed canonical(a + 1, 0).  The values canonical(a, R - 1), a = 2^25 + k, sit on such boundaries"""
    return [canonical(ol, 2 ** 25 + k, NMAX - 1) for k in range(n)]


def b1_probabilities(gl, ol, d=3):
    """walk b1_list until the library's threshold has a window of two high digits, place a = a_lo + 1 on draw d (closed form,
    engine offset 1) and take the outcome from kat_canonical; the first of each outcome is kept, the whole list is walked.
    -> ({"hit": (p, a, seed), "miss": ..}, every two-wide window walked as (p, a_lo, a_hi, b0, b1, b of the engine at a_lo + 1))

    Only misses exist.  The low digit is no free choice: x1 = x2 / 16807 mod M, so b = x1 - 1 < b1 needs x2 = 16807 x1 with
    x1 <= b1.  b1 is at most the rounding error of a R in units of 1, i.e. below ulp(a R) = 2^(k - 52) for a R ~ 2^k, which makes
    x2 <= 16807 b1 << a for every a >= 2^22: no engine state reaches the hit side of b1.  The CPU test asserts this on every
    window of the list instead of asserting that a hit exists"""
    found, windows = {}, []
    for p in b1_list(ol):
        a_lo, a_hi, b0, b1 = threshold(gl, p)
        if a_hi - a_lo != 2:
            continue
        a = a_lo + 1
        seed = solve_seed(d, a, 1)
        windows.append((p, a_lo, a_hi, b0, b1, digits(seed + 1, d)[1]))
        outcome = "hit" if draw_value(ol, seed + 1, d) < p else "miss"
        found.setdefault(outcome, (p, a, seed))
    return found, windows


def family_b(gl, ol):
    """the b1 outcomes that exist, as mutation tasks (engine offset 2; one chromosome per outcome, one map row each) and as
    crossover gametes for gev_dbg_sim_loc_rec"""
    d = 3
    found = b1_probabilities(gl, ol, d)[0]
    outcomes = [o for o in ("hit", "miss") if o in found]
    nchr, R = len(outcomes), 8
    rmaps, mmaps, gam = [], [], []
    mut_seeds = np.array([555 + t for t in range(3 * nchr)], dtype=np.int64)
    sc_claims = []
    for c, outcome in enumerate(outcomes):
        p, a, seed1 = found[outcome]
        bp, rprob, dist = rmap_rows(R)
        rp = rprob.copy(); rp[d] = p
        gam.append(((bp, rp, dist), seed1, d, outcome, (p, a)))
        mbp, mrate = mmap_rows(R + 1, int(bp[-1]))
        mrate[d + 1] = p
        rmaps.append((bp, rprob, dist)); mmaps.append((mbp, mrate))
        t = nchr + c                        # the second offspring's task on chromosome c
        mut_seeds[t] = solve_seed(d, a, 2, wrap=bool(c))
        sc_claims.append((t, "mut", outcome, d + 1))
    sc = Scenario("B b1", 3, rmaps, mmaps, 99, mut_seeds)
    sc.claims = sc_claims
    sc.designated = [(t, what, f"b1 {kind}") for t, what, kind, _ in sc_claims]
    sc.windows = [(found[k][0], found[k][1]) for k in outcomes]
    return sc.predict(ol), gam


# ---- family C: the edge of the candidate prefilter (closed form only) -------------------------------------
C_LARGE, C_SMALL = 2e-3, 1e-4


def family_c_points(gl):
    """(row kind, a, outcome or None = computed) for a map whose amax comes from one row at 2e-3 and whose designated row has 1e-4"""
    amax = threshold(gl, C_LARGE)[1]
    a_lo_small = threshold(gl, C_SMALL)[0]
    return [("small", amax - 1, "miss"), ("large", amax - 1, None), ("large", amax, "miss"), ("small", amax, "miss"), ("small", a_lo_small - 1, "hit")]


def family_c(gl, ol):
    """mutation tasks (reproduce) and crossover gametes (gev_dbg_sim_loc_rec) on the prefilter's edge"""
    R, row_l, row_s = 70, 5, 66
    bp, rprob, dist = rmap_rows(R)
    gp = rprob.copy(); gp[row_l] = C_LARGE; gp[row_s] = C_SMALL
    mbp, mrate = mmap_rows(R + 1, int(bp[-1]))
    mrate[row_l + 1] = C_LARGE; mrate[row_s + 1] = C_SMALL
    pts = family_c_points(gl)
    n_ind = len(pts) + 2
    mut_seeds = np.array([900 + t for t in range(n_ind)], dtype=np.int64)
    sc = Scenario("C prefilter edge", n_ind, [(bp, rprob, dist)], [(mbp, mrate)], 31, mut_seeds)
    gam = []
    for i, (kind, a, outcome) in enumerate(pts):
        d = row_l if kind == "large" else row_s
        t = 1 + i
        mut_seeds[t] = solve_seed(d, a, 2, wrap=bool(i & 1))
        if outcome is None:
            outcome = "hit" if draw_value(ol, int(mut_seeds[t]) + 2, d) < C_LARGE else "miss"
        sc.designated.append((t, "mut", f"{kind} row a={a}"))
        sc.claims.append((t, "mut", outcome, d + 1))
        s1 = solve_seed(d, a, 1, wrap=not (i & 1))
        o1 = pts[i][2] or ("hit" if draw_value(ol, s1 + 1, d) < C_LARGE else "miss")
        gam.append((s1, d, o1))
    sc.mut_seeds = mut_seeds.astype(np.uint32)
    return sc.predict(ol), ((bp, gp, dist), gam)


def family_c_all_candidates(ol, hit):
    """a row at p = 1.0 (amax at the top of the range: every draw is a candidate, and every scan hits that row) plus one straddled
    row, 300 rows: one scan holds more than 64 candidates"""
    R, row_one, d = 300, 150, 299
    bp, rprob, dist = rmap_rows(R)
    gp = rprob.copy(); gp[row_one] = 1.0
    s1 = solve_seed(d, 123_456_789, 1)
    _place(ol, gp, d, s1 + 1, d, hit)
    mbp, mrate = mmap_rows(R + 1, int(bp[-1]))
    mrate[row_one + 1] = 1.0
    mut_seeds = np.array([700 + t for t in range(4)], dtype=np.int64)
    mut_seeds[2] = solve_seed(d, 987_654_321, 2, wrap=True)
    _place(ol, mrate, d + 1, int(mut_seeds[2]) + 2, d, hit)
    sc = Scenario(f"C all candidates {'hit' if hit else 'miss'}", 4, [(bp, rprob, dist)], [(mbp, mrate)], 32, mut_seeds)
    sc.designated.append((2, "mut", "straddled row among candidates"))
    sc.claims += [(2, "mut", "hit" if hit else "miss", d + 1), (2, "mut", "hit", row_one + 1), (2, "mut", "count", 2 if hit else 1)]
    return sc.predict(ol), ((bp, gp, dist), [(s1, d, "hit" if hit else "miss"), (s1, row_one, "hit")])


# ---- family D: the counts at which a task leaves the fast path ------------------------------------------------
D_CASES = [("pat", 6), ("pat", 7), ("pat", 8), ("pat", 9), ("mat", 7), ("mat", 8), ("mut", 6), ("mut", 7), ("mut", 8), ("mut", 9)]


def family_d(ol, what, k):
    """task 0's paternal (k_pat = k) or maternal gamete (k_mat = k with k_pat = 0), or the mutations of task 2 (n_mut = k), with
    exactly k hits: the map is fitted to that one stream"""
    R, n_ind = 300, 5
    bp, rprob, dist = rmap_rows(R)
    mbp, mrate = mmap_rows(R + 1, int(bp[-1]))
    mut_seeds = np.array([4100 + 7 * t for t in range(n_ind)], dtype=np.int64)
    seed_reproduce = 5000 + k
    if what == "mut":
        mrate = fit_map_to_stream(ol, int(mut_seeds[2]) + 2, 1, R + 1, R, k)
        t = 2
    else:
        t = 0
        for seed_reproduce in range(5000 + 100 * k, 5000 + 100 * k + 50):
            r = oracle_api.kat_rand(ol, int(oracle_api.kat_rand(ol, seed_reproduce, 1)[0]), 2)
            sp = int(oracle_api.kat_rand(ol, seed_reproduce, 1)[0])
            if what == "pat":
                rprob = fit_map_to_stream(ol, sp + 1, 0, R, R, k)
                break
            rprob = fit_map_to_stream(ol, int(r[1]) + 1, 0, R, R, k)        # seed_mat if the paternal gamete has no crossover
            if not scan(ol, sp + 1, 0, rprob, R):
                break
        else:
            raise RuntimeError("family D: no reproduce seed leaves the paternal gamete without a crossover")
    sc = Scenario(f"D {what} k={k}", n_ind, [(bp, rprob, dist)], [(mbp, mrate)], seed_reproduce, mut_seeds)
    sc.designated.append((t, what, f"{k} records"))
    sc.claims.append((t, what, "count", k))
    if what == "mat":
        sc.designated.append((t, "pat", "no crossover")); sc.claims.append((t, "pat", "count", 0))
    return sc.predict(ol)


# ---- family E: where in a wave batch of eight the task sits ------------------------------------------------------
E_SHAPES = [(1, 17), (1, 18), (3, 11), (3, 6)]          # (nchr, n_ind): 17, 18, 33, 18 tasks = 1, 2, 1, 2 (mod 8)


def family_e(ol, nchr, n_ind, what):
    """a placed hit (draw 5 of 70) in the paternal gamete ("pat": producer seeds searched) or in the mutation scan ("mut": closed
    form) of tasks 0, 1, 7, 8, 9 and the last one"""
    R, d = 70, 5
    n_tasks = nchr * n_ind
    ts = sorted({0, 1, 7, 8, 9, n_tasks - 1})
    rmaps = [rmap_rows(R) for _ in range(nchr)]
    mmaps = [mmap_rows(R + 1, int(rmaps[0][0][-1])) for _ in range(nchr)]
    mut_seeds = np.array([8000 + 31 * t for t in range(n_tasks)], dtype=np.int64)
    seed_reproduce = 61
    sc_des = []
    # one placed row per designated task: rows d, d + 1, .. of its chromosome's map, so that no two tasks share a row
    for i, t in enumerate(ts):
        c, di = t % nchr, d + i
        if what == "mut":
            mut_seeds[t] = solve_seed(di, _a_target(i), 2, wrap=bool(i & 1))
            _place(ol, mmaps[c][1], di + 1, int(mut_seeds[t]) + 2, di, True)
            sc_des.append((t, "mut", di + 1))
        else:
            prod = _producer(ol, mmaps, nchr, t - 1)
            if t == 0:
                seed_reproduce = S = search_seed(61, prod, di)
            else:
                mut_seeds[t - 1] = S = search_seed(30_000 + 1000 * t, prod, di)
            _place(ol, rmaps[c][1], di, prod(S) + 1, di, True)
            sc_des.append((t, "pat", di))
    sc = Scenario(f"E nchr={nchr} n_ind={n_ind} {what}", n_ind, rmaps, mmaps, seed_reproduce, mut_seeds)
    for t, w, row in sc_des:
        sc.designated.append((t, w, f"row {row}")); sc.claims.append((t, w, "hit", row))
    return sc.predict(ol)


# ---- the case list (built once per process; both test files take their cases from here) ------------------------------
import functools
import itertools


@functools.lru_cache(maxsize=None)
def libs():
    """(product library: host-side threshold construction only, oracle)"""
    from geneevolve_amd.capi import GevLibrary
    return GevLibrary(), oracle_api.load()


VARIANTS = list(itertools.product((True, False), (False, True)))      # (hit, warm)
REPRODUCE_GROUPS = [f"A{n}" for n in N_DRAWS] + ["BC", "D", "E"]
CHAIN_GROUPS = [f"A{n}" for n in N_DRAWS[1:]] + ["D"]
GAMETE_GROUPS = [f"A{n}" for n in N_DRAWS[1:]] + ["BC"]


@functools.lru_cache(maxsize=None)
def reproduce_scenarios(group):
    """scenarios with a mutation map (k_sample_batched, or k_mut_sample + k_rec_sample)"""
    gl, ol = libs()
    if group[0] == "A":
        return [family_a(ol, int(group[1:]), hit, warm) for hit, warm in VARIANTS]
    if group == "BC":
        return [family_b(gl, ol)[0], family_c(gl, ol)[0], family_c_all_candidates(ol, True)[0], family_c_all_candidates(ol, False)[0]]
    if group == "D":
        return [family_d(ol, what, k) for what, k in D_CASES]
    return [family_e(ol, nchr, n_ind, what) for nchr, n_ind in E_SHAPES for what in ("pat", "mut")]


@functools.lru_cache(maxsize=None)
def chain_scenarios(group):
    """scenarios without a mutation map (k_rec_chain_wg / k_rec_chain): crossover families, the designated gamete in task 0"""
    gl, ol = libs()
    if group[0] == "A":
        n = int(group[1:])
        return [family_a_task0(ol, n, d, hit, warm) for d in edge_draws(n) for hit, warm in VARIANTS]
    return [sc.without_mutation(sc.name + " chain").predict(ol) for sc in reproduce_scenarios("D") if sc.designated[0][1] != "mut"]


@functools.lru_cache(maxsize=None)
def gamete_cases(group):
    """gev_dbg_sim_loc_rec form: [(name, rmap, [(seed, row, "hit" / "miss")], [(p, a)] window claims)]"""
    gl, ol = libs()
    if group[0] == "A":
        out = []
        for hit, warm in VARIANTS:
            rmap, seeds, windows = gamete_cases_a(ol, int(group[1:]), hit, warm)
            out.append((f"A n={group[1:]} {'hit' if hit else 'miss'} {'warm' if warm else 'cold'}", rmap,
                        [(s, d, "hit" if hit else "miss") for s, d in seeds], windows))
        return out
    out = [(f"B b1 {o}", rmap, [(seed, d, o)], [w]) for rmap, seed, d, o, w in family_b(gl, ol)[1]]
    rmap, gam = family_c(gl, ol)[1]
    out.append(("C prefilter edge", rmap, gam, []))
    for hit in (True, False):
        rmap, gam = family_c_all_candidates(ol, hit)[1]
        out.append((f"C all candidates {'hit' if hit else 'miss'}", rmap, gam, []))
    return out
