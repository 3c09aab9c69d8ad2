// gev_sample8.h -- batched crossover / mutation sampling (K1-K3), gfx950 wave64.  Included by gev_kernels.h.
//
// Same arithmetic as the one-task-per-wave kernels of gev_kernels.h (k_mut_sample, k_rec_sample: bit-exact restatements of
// Simulation::ras_add_mutation, src/Simulation.cpp:2497-2552, and Simulation::ras_sim_loc_rec, :2973-2995, with the rand()
// chain of Simulation::reproduce, :2447-2455), reorganised so that the per-task fixed costs are shared by EIGHT tasks:
//
//   * srand(): the glibc TYPE_3 generator is linear, output j = sum_i W[i][j] * r_i (mod 2^32).  The old form evaluates all 64
//     outputs of one generator per wave (31 multiply steps) and uses ~3 of them.  Here lane (g, j) = (lane >> 3, lane & 7) holds
//     output j of generator g: ONE pass of 31 multiply steps yields the first 8 outputs of 8 generators.
//   * map scan: the same lane grid.  Lane (g, j) owns draws j, j + 8, ... of task g, so ONE loop scans the maps of all eight
//     tasks (see scan_candidates); only the high digit of generate_canonical is produced per draw and compared with the map's
//     largest a_hi, and a candidate is only RECORDED (row, high digit, task) in an LDS list.
//   * resolve: the candidates of all 8 scans are tested against their threshold rows lane-parallel (one 16-byte load per
//     candidate instead of a divergent load inside the scan loop), hits are ranked per task with ballots, and the per-hit work
//     (breakpoint = bp[row] + rand() % dist; mutation position by uniform_int_distribution, side = rand() % 2) runs one hit per
//     lane.
//
// One kernel (k_sample_batched) samples a generation's mutations and gametes: wave b takes the mutations of tasks [8b, 8b+8),
// then both gametes of tasks [8b+1, 8b+9), whose paternal seeds come out of the mutation streams it has just run.  A task
// that needs more than the 8 precomputed rand() outputs (k + 2 > 8 crossovers / mutations), or whose mutation position draw
// hits the rejection branch of uniform_int_distribution, is finished by the same wave with the one-task-per-wave arithmetic
// (expected: ~1e-4 of the tasks at one event per gamete).
#pragma once

#define SB_TASKS 8          // tasks per wave batch
#define SB_OUT 8            // rand() outputs per generator held in the lane grid
#define SB_CAND 320         // candidate slots per wave: a flush is forced at >= 64, one scan step adds <= 256

#define SB_M 256            // draws per lane that are prefiltered from ONE exact engine state
#define SB_BLK (8 * SB_M)   // draws of one task per block: 8 lanes x SB_M
#define SB_RSTRIDE 36       // words per row of the srand8 operands (31 used, the 32nd is padding): rows start on 16 bytes and, at 144
                            // bytes apart, the eight rows of a 16-byte read fall on eight different bank quads (0, 36, 8, 44, 16, 52, 24, 60)
// FP64 prefilter of the scan (derivation: scan_candidates).  The fraction field is the SB_PF_BITS low mantissa bits of the FMA; with
// F = floor(x2 * 2^16 / M) the field is L = F + SB_PF_OFF + d (mod 2^16) with -SB_PF_DNEG <= d <= SB_PF_DPOS, which
// gev_dbg_prefilter_sweep checks exhaustively with these very constants.  The offset keeps L from wrapping below 0, the margin is
// what a draw with F = floor(A) can reach, plus one for the strict compare.
#define SB_PF_BITS 16
#define SB_PF_DNEG 0
#define SB_PF_DPOS 1
#define SB_PF_OFF SB_PF_DNEG
#define SB_PF_MARGIN (SB_PF_OFF + SB_PF_DPOS + 1u)
#define SB_PF_ONE 65536.0                                              // 2^SB_PF_BITS
#define SB_PF_MASK 0xffffu
#define SB_PF_BIAS (103079215104.0 + (double)SB_PF_OFF / SB_PF_ONE)    // 1.5 * 2^36 + offset: ulp = 2^-16 = one unit of the field
struct __attribute__((aligned(32))) SmpTabs {   // constant tables, one copy per workgroup (LDS)
    double kd[SB_M + 4];    // c_m / M with c_m = 16807^(16 m) mod M: draw (j + 8 m)'s high digit = x_j * c_m mod M; 4 spare entries
                            // (0) behind the last one, so that the scan may always load the next step's four
    u32 ci[SB_M];           // c_m
    u32 pow_even[64];       // 16807^(2l+2): draw l's high-digit engine output
    u32 w8[SB_OUT * SB_RSTRIDE];   // row j < 8: w_init[i][j], i < 31, then 0
    u32 pow_lcg[32];        // 16807^(i-1), i = 1..30
    u32 pow_blk /* 16807^(2 SB_BLK): next block of draws */, inv16807, pad[2];
};
struct __attribute__((aligned(16))) SmpWave {   // scratch of one wave (LDS)
    u32 r[SB_TASKS * SB_RSTRIDE];   // row g: seed words r_0..r_30 of generator g, then one padding word
    u32 cand_row[SB_CAND];
    u32 cand_x2[SB_CAND];
    uint8_t cand_tag[SB_CAND];
};

__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
__device__ __forceinline__ u32 mbcnt64(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u)); }

// Multiplier m < SB_M of the scan, c_m = 16807^(16 m) mod M (8 draws = 16 engine steps; 16807^16 is pow_even[7]), and the FP64
// constant fl(c_m / M) the prefilter multiplies with.  The one definition for the kernel's tables and for the exhaustive check.
__device__ __forceinline__ void smp_scan_multiplier(const GevRngTables* __restrict__ g, u32 m, u32& c, double& k)
{
    c = powmod31(g->pow_even[7], m);
    k = (double)c / 2147483647.0;
}

__device__ __forceinline__ void stage_smp_tabs(const GevRngTables* __restrict__ g, SmpTabs* s)
{
    for (u32 i = threadIdx.x; i < 64; i += blockDim.x) s->pow_even[i] = g->pow_even[i];
    for (u32 i = threadIdx.x; i < SB_OUT * 32; i += blockDim.x) s->w8[(i >> 5) * SB_RSTRIDE + (i & 31u)] = (i & 31u) < 31u ? g->w_init[(i & 31u) * 64 + (i >> 5)] : 0u;
    for (u32 i = threadIdx.x; i < 31; i += blockDim.x) s->pow_lcg[i] = g->pow_lcg[i];
    for (u32 i = threadIdx.x; i < SB_M; i += blockDim.x) smp_scan_multiplier(g, i, s->ci[i], s->kd[i]);
    if (threadIdx.x < 4) s->kd[SB_M + threadIdx.x] = 0.0;
    if (threadIdx.x == 0) { s->pow_lcg[31] = 0; s->pow_blk = powmod31(g->pow_even[7], SB_M); s->inv16807 = g->inv16807; s->pad[0] = s->pad[1] = 0; }
    __syncthreads();
}

// srand(seed) for eight generators at once: every lane of group g passes generator g's seed; returns raw output word j = lane & 7
// of generator g = lane >> 3 (rand() = word >> 1).  Same seeding arithmetic as GlibcWave::seed: r_0 = seed (0 -> 1), r_1 by the
// signed Schrage step of random_r.c (a seed >= 2^31 enters as a negative int32; every intermediate fits 32 bits: |lo| < 127773
// and |hi| <= 16807 give |16807 lo - 2836 hi| < 2^31), r_i = 16807^(i-1) r_1 mod M.  Each lane takes the step for its own group's
// seed once and writes the words i = j, j + 8, j + 16, j + 24 of its group's generator (i = 31, lane 7's last: pow_lcg[31] = 0, the
// row's padding word); then lane (g, j) sums row j of w8 against row g of Wr, both read 16 bytes at a time.  Wr is plain LDS
// between two wave fences, like the candidate lists.
__device__ __forceinline__ u32 srand8(const SmpTabs* __restrict__ T, u32* __restrict__ Wr, u32 seed)
{
    const u32 lane = threadIdx.x & 63, g = lane >> 3, j = lane & 7u;
    const u32 sv = seed == 0 ? 1u : seed;
    const int32_t w0 = (int32_t)sv;
    const int32_t hi = w0 / 127773, lo = w0 % 127773;
    int32_t w = 16807 * lo - 2836 * hi;
    if (w < 0) w += 2147483647;
    u32* row = Wr + g * SB_RSTRIDE;
#pragma unroll
    for (u32 p = 0; p < 4; p++) {
        const u32 i = j + 8u * p;
        const u32 val = mulmod31(T->pow_lcg[i], (u32)w);
        row[i] = i == 0 ? sv : val;
    }
    wave_fence();
    const uint4* wq = reinterpret_cast<const uint4*>(T->w8 + j * SB_RSTRIDE);
    const uint4* rq = reinterpret_cast<const uint4*>(row);
    u32 acc = 0;
#pragma unroll
    for (u32 q = 0; q < 8; q++) {
        const uint4 a = wq[q], b = rq[q];
        acc += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    }
    wave_fence();
    return acc;
}

// The Bernoulli scans of the wave's EIGHT tasks in one loop, on the lane grid of srand8.  All arguments but T, W, count and flush
// are per-lane values, equal within a lane group: task g = lane >> 3 draws from engine = minstd_rand0(engine_seed), its draw d
// tests map row first_row + d, d < n_draws (0: the task has no scan), and a draw whose high digit x2 - 1 is below `amax` (the
// largest a_hi of the task's map) is only RECORDED: it goes to the wave's candidate list, tagged g.  `count` (wave-uniform) is
// the list length; `flush()` must consume the list and reset count when it reaches 64.
//
// Layout.  Lane (g, j) owns draws j, j + 8, j + 16, ... of task g.  It holds ONE exact engine state x per block of SB_BLK = 2048
// draws of its task, the high digit of draw j of the block (engine output 2 j + 2: pow_even[j]); the high digit of its draw
// j + 8 m is x * c_m mod M with c_m = 16807^(16 m), m < SB_M = 256, and the next block starts from x * 16807^4096.  One step of
// the loop tests four m, that is 32 draws of each of the eight tasks, with wave-uniform constants c_m / M (one broadcast 32-byte
// LDS read per step, issued one step ahead of its use; two steps ahead measured the same, and broadcasting the constants from
// lanes with v_readlane measured 33 % slower in the earlier layout).  The tasks' ranges may differ (chromosomes with different maps, tasks
// off the fast path): the loop runs without bounds tests while every lane that has draws left in the block is inside its
// range, then with a per-lane bound up to the longest range; a lane without draws in the block carries the threshold 0, which
// no draw passes.
//
// Order.  rank_hits needs the candidates of one task in ascending draw order.  Candidates are pushed step by step, within a
// step m by m, and within one m in lane order; for one task, (m, j) ascending is draw 8 m + j ascending.
//
// FP64 prefilter.  The high digit of draw j + 8 m is x2 = x * c_m mod M, i.e. M * frac(T) with T = x * c_m / M < 2^31.  One FMA
// evaluates
//     s = x * fl(c_m / M) + 1.5 * 2^36,   u = 2^-16 = ulp(s),
// whose 16 low mantissa bits are  L = round(y + e) mod 2^16,  y = frac(T) * 2^16 = x2 * 2^16 / M,  where e is the error of the
// rounded constant alone, |e| <= 2^-22 absolute = 2^-6 u (the bound holds for any multiplier below M), and round() is the one
// rounding of the FMA to a multiple of u.  With F = floor(y): y is no integer (M is prime) and lies at least 2^-31 from one, so
// y + e stays inside (F - 1/2, F + 3/2) and  L = F + d,  d in {0, 1}.  A draw with x2 <= amax has F <= floor(A), A = amax * 2^16 / M,
// hence L <= floor(A) + 1: it passes  L < floor(A) + 2  (SB_PF_MARGIN; no offset is needed, because d is never negative; the 20-bit
// field this replaces carried an offset of 4 and a margin of 7, which the same argument and the sweep's extremes show to be more
// than needed).  floor(A) is exact in FP64: A is no integer either, at least 2^-31 from one, and the two roundings of its
// evaluation move it by less than 2^-35.  Where floor(A) + 2 >= 2^16 every draw is a candidate.  The field is 16 bits wide so that
// the mask folds into the compare (v_cmp_lt_u32_sdwa on WORD_0): the test is ONE v_fma_f64 and ONE compare per 64 draws, against
// a 10-instruction modular multiply for the exact form.  It is a SUPERSET of the exact test, 1 to 2 units of 2^-16 wide beyond A
// (~2.3e-5 of the draws: 5 % extra candidates at 5e-4 per row); every candidate's exact x2 is then computed with the integer
// multiply and the exact threshold test runs in the resolve step, so the result is bit-identical.  gev_dbg_prefilter_sweep checks
// d in [-SB_PF_DNEG, SB_PF_DPOS] exhaustively over all 2^31 - 2 engine states x 256 multipliers, with the kernel's own constants.
template <class Flush>
__device__ __forceinline__ void scan_candidates(const SmpTabs* __restrict__ T, SmpWave* __restrict__ W, u32 engine_seed, u32 amax,
                                                u32 first_row, u32 n_draws, u32& count, Flush&& flush)
{
    const u32 lane = threadIdx.x & 63, g = lane >> 3, j = lane & 7u;
    if (amax == 0) n_draws = 0;                            // every row has probability 0: no draw can hit
    u32 n_max = 0;                                         // the longest scan of the eight
#pragma unroll
    for (u32 q = 0; q < SB_TASKS; q++) n_max = max(n_max, rl_u32(n_draws, q * 8u));
    if (n_max == 0) return;
    u32 x = mulmod31(T->pow_even[j], minstd_seed(engine_seed));   // exact high digit (engine output 2 j + 2) of draw j
    const double A = (double)amax * (SB_PF_ONE / 2147483647.0);      // floor(A) is exact: see the header comment
    const bool all_cand = A + (double)SB_PF_MARGIN >= SB_PF_ONE;     // thresholds near 1: every draw is a candidate
    const u32 thr_pf = all_cand ? 0xffffffffu : (u32)A + SB_PF_MARGIN;
    double C = SB_PF_BIAS;
    asm volatile("" : "+s"(C));                            // wave-uniform: lives in a scalar register pair, which the FMA reads directly (left to
                                                           // itself the compiler rebuilds it in vector registers with two moves per half-step)
    for (u32 base = 0; base < n_max; base += SB_BLK) {
        const u32 n_here = n_draws > base ? min((u32)SB_BLK, n_draws - base) : 0u;   // draws of the lane's task in this block
        const u32 cnt = n_here > j ? (n_here - j + 7u) >> 3 : 0u;                    // ... of which the lane owns m < cnt
        const u32 thr = cnt ? thr_pf : 0u;
        u32 n_lo = SB_BLK, n_hi = 0;                       // shortest non-empty and longest range of the eight tasks
#pragma unroll
        for (u32 q = 0; q < SB_TASKS; q++) { const u32 nq = rl_u32(n_here, q * 8u); n_hi = max(n_hi, nq); if (nq) n_lo = min(n_lo, nq); }
        const u32 m_all = n_lo >= 8u ? n_lo >> 3 : 1u;     // every lane with cnt != 0 has cnt >= m_all (its smallest: lane min(7, n_lo - 1))
        const u32 m_end = (n_hi + 7u) >> 3;                // the largest cnt (lane 0 of the longest task)
        const double xd = (double)x;
        const u32 row0 = first_row + base + j;
        auto testk = [&](double k) -> bool { return ((u32)__double2loint(__fma_rn(xd, k, C)) & SB_PF_MASK) < thr; };
        auto push = [&](unsigned long long mk, bool c, u32 m) {
            if (c) {
                const u32 idx = count + mbcnt64(mk);
                W->cand_row[idx] = row0 + 8u * m;
                W->cand_x2[idx] = mulmod31(x, T->ci[m]);  // the exact high digit of this draw
                W->cand_tag[idx] = (uint8_t)g;
            }
            count += (u32)__popcll(mk);
        };
        // four m (32 draws of every task) per step; a step tests with the constants c_m / M in `k` and loads the next step's
        // into `kn` first (two register sets that take turns, so that nothing is copied)
        auto step = [&](u32 m, const double4& k, double4& kn, const bool bounded) {
            kn = *reinterpret_cast<const double4*>(&T->kd[m + 4]);
            const bool c0 = (!bounded || m < cnt) && testk(k.x), c1 = (!bounded || m + 1 < cnt) && testk(k.y),
                       c2 = (!bounded || m + 2 < cnt) && testk(k.z), c3 = (!bounded || m + 3 < cnt) && testk(k.w);
            const unsigned long long m0 = __ballot(c0), m1 = __ballot(c1), m2 = __ballot(c2), m3 = __ballot(c3);
            if (m0 | m1 | m2 | m3) {
                push(m0, c0, m); push(m1, c1, m + 1); push(m2, c2, m + 2); push(m3, c3, m + 3);
                if (count >= 64) flush();
            }
        };
        double4 ka = *reinterpret_cast<const double4*>(&T->kd[0]), kb;
        u32 m = 0;
        for (; m + 8 <= m_all; m += 8) { step(m, ka, kb, false); step(m + 4, kb, ka, false); }   // every lane in range (or empty): no bounds to check
        for (; m < m_end; m += 4) { step(m, ka, kb, true); ka = kb; }                            // the ends of the ranges
        if (base + SB_BLK < n_max) x = mulmod31(x, T->pow_blk);
    }
}

// rank of a hit among the hits of its own task: hits so far (lane-held per group in `hc`) + earlier hit lanes with the same tag.
// Updates hc.  `valid`/`tg`/`hit` are per lane; all lanes must call.
__device__ __forceinline__ u32 rank_hits(bool valid, u32 tg, bool hit, u32& hc)
{
    const u32 lane = threadIdx.x & 63, g = lane >> 3;
    u32 h = 0;
#pragma unroll
    for (u32 q = 0; q < SB_TASKS; q++) {
        const unsigned long long mq = __ballot(valid && hit && tg == q);
        const u32 base = rl_u32(hc, q * 8u);
        if (tg == q) h = base + mbcnt64(mq);
        if (g == q) hc += (u32)__popcll(mq);
    }
    return h;
}


// ------------------------------------------------------------------------------------------
// K1-K3 batched, one kernel: wave b samples the mutations of tasks [8b, 8b+8) (Simulation::ras_add_mutation), then both
// gametes of tasks [8b+1, 8b+9) (ras_sim_loc_rec, :2447-2455).  The paternal seed of task t+1 is a rand() of task t's mutation
// stream, so lane group g hands it to the gamete phase in a register; only task 0 takes its seed from srand(seed_reproduce)
// (:2400, :2447), and batch 0 samples its gametes in a pass of their own before the others.  A task that needs more than
// SB_OUT rand() outputs or hits the rejection branch of uniform_int_distribution is finished by the same wave, one task at a
// time, with the one-task-per-wave arithmetic (mut_task / rec_task on the global tables) behind a wave-uniform branch.
// ------------------------------------------------------------------------------------------
// The slow tasks, out of line: their arithmetic needs far more registers than the batched loop, and called where little is live
// they do not cost the loop its occupancy
__device__ __noinline__ void slow_rec_task(const GevRngTables* __restrict__ Tg, const ChrDev* __restrict__ chrs, u32 c, u32 seed_pat, size_t t, const SampleDev& sd)
{
    rec_task(Tg, chrs[c], seed_pat, t, sd);
}
__device__ __noinline__ void slow_mut_task(const GevRngTables* __restrict__ Tg, const ChrDev* __restrict__ chrs, const u32* __restrict__ mut_seeds, u32 nchr,
                                           size_t t, size_t n_tasks, const SampleDev& sd)
{
    const u32 c = (u32)(t % nchr);
    const u32 nxt = mut_task(Tg, chrs[c], c == nchr - 1, mut_seeds[t], t, sd, nchr);
    if (t + 1 < n_tasks) rec_task(Tg, chrs[(t + 1) % nchr], nxt, t + 1, sd);        // the gametes of the task behind it
}
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7))) k_sample_batched(const GevRngTables* __restrict__ Tg, const ChrDev* __restrict__ chrs, int nchr,
                                                        const u32* __restrict__ mut_seeds, u32 seed_reproduce, const u32* __restrict__ seed_ptr,
                                                        size_t n_tasks, SampleDev sd)
{
    __shared__ SmpTabs s_T;
    __shared__ SmpWave s_W[4];
    stage_smp_tabs(Tg, &s_T);
    const SmpTabs* T = &s_T;
    SmpWave* W = &s_W[threadIdx.x >> 6];
    const u32 lane = threadIdx.x & 63, g = lane >> 3, j = lane & 7u;
    const size_t n_batches = (n_tasks + SB_TASKS - 1) / SB_TASKS;
    for (size_t b = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n_batches; b += (size_t)gridDim.x * 4) {
        // ---- mutations of task t = 8b + g
        const size_t t = b * SB_TASKS + g;
        const bool valid = t < n_tasks;
        const u32 cidx = valid ? (u32)(t % (size_t)nchr) : 0u;
        const u32 S = valid ? mut_seeds[t] : 1u;
        u32 seed0 = 0;
        if (b == 0) {                                       // first rand() after srand(seed) of reproduce (:2400, :2447) = seed_loc of task 0
            const u32 x0 = srand8(T, W->r, seed_ptr ? *seed_ptr : seed_reproduce);
            seed0 = rl_u32(x0, 0) >> 1;
            if (lane == 0) sd.seed_pat[0] = seed0;
        }
        u32 seed_next;                                      // seed_pat[t + 1]: lane group g's paternal seed in the gamete phase
        bool slow_mut;                                      // ... unless task t is slow: then task t + 1's gametes are late too
        {
            const u32 xout = srand8(T, W->r, S);           // srand(seed), :2501
            u32 hc = 0, count = 0;
            bool rej = false;
            auto resolve = [&]() {
                wave_fence();
                for (u32 c0 = 0; c0 < count; c0 += 64) {
                    const u32 idx = c0 + lane; const bool cv = idx < count;
                    const u32 row = cv ? W->cand_row[idx] : 1u, x2 = cv ? W->cand_x2[idx] : 1u, tg = cv ? (u32)W->cand_tag[idx] : 0u;
                    const u32 cq = (u32)__shfl((int)cidx, (int)(tg * 8u));
                    const u32 Sq = (u32)__shfl((int)S, (int)(tg * 8u));
                    const ChrDev& C = chrs[cq];
                    bool hit = false;
                    if (cv) { const GevThr th = C.mthr[row]; hit = thr_hit(th, mulmod31(x2, T->inv16807), x2); }
                    const u32 h = rank_hits(cv, tg, hit, hc);
                    const u32 o = (u32)__shfl((int)xout, (int)(tg * 8u + (h < SB_OUT ? h : SB_OUT - 1u)));
                    bool rj = false;
                    if (hit && h < GEV_NM_CAP) {
                        // uniform_int_distribution<unsigned long>(bp[i-1], bp[i]) on generator(seed+1), :2503, :2516-2520: hit h of a task
                        // takes engine output h+1 as long as no earlier draw of the task was rejected
                        const u32 x = mulmod31(T->pow_lcg[h + 2], minstd_seed(Sq + 1u));
                        const u64 lo = C.mbp[row - 1], hi = C.mbp[row];
                        const u32 uerange = (u32)(hi - lo) + 1u;                   // < 2147483645 (checked by gev_set_mutmap)
                        const u32 scaling = 2147483645u / uerange, past = uerange * scaling, ret = x - 1u;
                        rj = ret >= past;
                        const size_t slot = (size_t)(b * SB_TASKS + tg) * GEV_NM_CAP + h;
                        sd.nm_pos[slot] = (u64)(ret / scaling) + lo;
                        sd.nm_side[slot] = (uint8_t)((o >> 1) & 1u);                // rand()%2, :2522
                    }
#pragma unroll
                    for (u32 q = 0; q < SB_TASKS; q++) { const unsigned long long mr = __ballot(rj && tg == q); if (g == q && mr) rej = true; }
                }
                count = 0;
                wave_fence();
            };
            {
                const ChrDev& C = chrs[cidx];
                const u32 M = valid ? C.M : 0u;
                scan_candidates(T, W, S + 2u, C.m_amax, 1u, M >= 2 ? M - 1u : 0u, count, resolve);   // generator_u(seed+2), i = 1..M-1
            }
            if (count) resolve();
            const u32 n = hc;
            const bool last = cidx == (u32)(nchr - 1);
            const bool slow = valid && (n + 2u > SB_OUT || rej);
            const u32 o_sex = (u32)__shfl((int)xout, (int)(g * 8u + (n < SB_OUT ? n : SB_OUT - 1u)));
            const u32 n2 = n + (last ? 1u : 0u);
            const u32 o_nxt = (u32)__shfl((int)xout, (int)(g * 8u + (n2 < SB_OUT ? n2 : SB_OUT - 1u)));
            seed_next = o_nxt >> 1;                                                                 // seed_loc of the next task, :2447
            if (valid && j == 0 && !slow) {
                sd.nmut[t] = n; sd.nm_off[t] = (u32)t * GEV_NM_CAP;
                if (last) sd.sex[t / (size_t)nchr] = (uint8_t)(((o_sex >> 1) & 1u) + 1u);      // :2472
                sd.seed_pat[t + 1] = seed_next;
            }
            slow_mut = slow;
        }
        // ---- both gametes of task t0 + g: t0 = 0 (task 0 alone, batch 0 only), then t0 = 8b + 1
#pragma unroll 1
        for (u32 pass = b == 0 ? 0u : 1u; pass < 2; pass++) {
            const size_t t0 = pass ? b * SB_TASKS + 1 : 0, tr = t0 + g;
            const bool rvalid = pass ? tr < n_tasks : g == 0;
            const u32 rc = rvalid ? (u32)(tr % (size_t)nchr) : 0u;
            const bool active = rvalid && chrs[rc].active != 0;       // inactive: another context owns this chromosome (only the seed chain is needed)
            const u32 R = chrs[rc].R, r_amax = chrs[rc].r_amax;       // the map of both gametes' scans
            const u32 seed_pat = pass ? seed_next : seed0;
            const bool late = pass && slow_mut;
            u32 seed_cur = seed_pat, xout = 0, hc = 0, count = 0, side = 0;
            bool run = active && !late;
            auto resolve = [&]() {
                wave_fence();
                for (u32 c0 = 0; c0 < count; c0 += 64) {
                    const u32 idx = c0 + lane; const bool cv = idx < count;
                    const u32 row = cv ? W->cand_row[idx] : 0u, x2 = cv ? W->cand_x2[idx] : 1u, tg = cv ? (u32)W->cand_tag[idx] : 0u;
                    const u32 cq = (u32)__shfl((int)rc, (int)(tg * 8u));
                    const ChrDev& C = chrs[cq];
                    bool hit = false;
                    if (cv) { const GevThr th = C.rthr[row]; hit = thr_hit(th, mulmod31(x2, T->inv16807), x2); }
                    const u32 h = rank_hits(cv, tg, hit, hc);
                    const u32 o = (u32)__shfl((int)xout, (int)(tg * 8u + (h < SB_OUT ? h : SB_OUT - 1u)));
                    if (hit && h < GEV_BK_CAP) {
                        const u32 rv = o >> 1;                                                        // rand(), :2990
                        const u64 dist = C.bp_dist;
                        const u64 v = C.rbp[row] + (dist > 0x7fffffffull ? (u64)rv : (u64)(rv % (u32)dist));
                        const size_t G = 2 * (t0 + tg) + side;
                        sd.bk[G * GEV_BK_CAP + h] = v;
                        sd.bk_idx[G * GEV_BK_CAP + h] = snp_lower_bound(C, v);     // first locus at or behind the breakpoint (what the dense stitch and the unit table work with)
                    }
                }
                count = 0;
                wave_fence();
            };
            auto phase = [&]() {                           // ras_sim_loc_rec for the current gamete of every task that is still on the fast path
                xout = srand8(T, W->r, seed_cur);          // srand(seed), :2977
                hc = 0; count = 0;
                scan_candidates(T, W, seed_cur + 1u, r_amax, 0u, run ? R : 0u, count, resolve);   // generator(seed+1), :2978
                if (count) resolve();
            };
            // paternal gamete (:2447-2449)
            side = 0; phase();
            const u32 k_pat = hc;
            bool slow = run && k_pat + 2u > SB_OUT;
            const u32 o_sp = (u32)__shfl((int)xout, (int)(g * 8u + (k_pat < SB_OUT ? k_pat : SB_OUT - 1u)));
            const u32 o_sm = (u32)__shfl((int)xout, (int)(g * 8u + (k_pat + 1u < SB_OUT ? k_pat + 1u : SB_OUT - 1u)));
            const u32 start_pat = (o_sp >> 1) & 1u;        // rand()%2 after k_pat position draws, :2449
            const u32 seed_mat = o_sm >> 1;                // :2453
            // maternal gamete (:2453-2455)
            run = run && !slow; seed_cur = seed_mat;
            side = 1; phase();
            const u32 k_mat = hc;
            slow = slow || (run && k_mat + 1u > SB_OUT);
            const u32 o_st = (u32)__shfl((int)xout, (int)(g * 8u + (k_mat < SB_OUT ? k_mat : SB_OUT - 1u)));
            const u32 start_mat = (o_st >> 1) & 1u;        // :2455
            if (rvalid && j == 0 && !late) {
                if (!active) {
                    sd.k[2 * tr] = 0; sd.k[2 * tr + 1] = 0; sd.bk_off[2 * tr] = (u32)(2 * tr) * GEV_BK_CAP; sd.bk_off[2 * tr + 1] = (u32)(2 * tr + 1) * GEV_BK_CAP;
                    sd.start[2 * tr] = 0; sd.start[2 * tr + 1] = 0; sd.seed_mat[tr] = 0;
                } else if (!slow) {
                    sd.k[2 * tr] = k_pat; sd.k[2 * tr + 1] = k_mat; sd.bk_off[2 * tr] = (u32)(2 * tr) * GEV_BK_CAP; sd.bk_off[2 * tr + 1] = (u32)(2 * tr + 1) * GEV_BK_CAP;
                    sd.start[2 * tr] = (uint8_t)start_pat; sd.start[2 * tr + 1] = (uint8_t)start_mat; sd.seed_mat[tr] = seed_mat;
                }
            }
            unsigned long long ms = __ballot(slow && j == 0);
            if (ms) {                                       // rare: both gametes once more, one task per wave, in place
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");        // the records the batched pass wrote land first
                while (ms) {
                    const u32 q = (u32)(__ffsll((long long)ms) - 1) >> 3;
                    ms &= ms - 1;
                    slow_rec_task(Tg, chrs, rl_u32(rc, q * 8u), rl_u32(seed_pat, q * 8u), t0 + q, sd);
                }
            }
        }
        // rare: a slow mutation task once more, one task per wave, then the gametes of the task behind it (its seed is known now)
        unsigned long long ms = __ballot(slow_mut && j == 0);
        if (ms) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            while (ms) {
                const u32 q = (u32)(__ffsll((long long)ms) - 1) >> 3;
                ms &= ms - 1;
                slow_mut_task(Tg, chrs, mut_seeds, (u32)nchr, b * SB_TASKS + q, n_tasks, sd);
            }
        }
    }
}
