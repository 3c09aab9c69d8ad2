// gev_assort.h -- Simulation::assort_mate (reference src/Simulation.cpp:2167-2360) on the device (gfx950, wave64).  Included by
// gev_kernels.h after gev_mate.h and gev_normal.h.  The host mirror geneevolve_amd/host.py:assort_mate is the specification; every
// stream below is reproduced bit for bit (DESIGN.md "Assortative mating on the device" has the exactness arguments).
//
//   :2184-2216  marriage draws      k_am_chunk_stats / k_am_windows / k_am_walk / k_am_chain / k_am_flags / k_am_compact
//   :2232-2246  surplus removal     k_glibc_stream + k_shuf_count / k_shuf_fill / k_shuf_trace (std::random_shuffle on rand())
//   :2251-2252  sort by mv          gev_sort_pairs_f64 (gev_sort.hip, stable radix sort)
//   :2257-2275  template            k_tpl_count / k_tpl_emit (ras_mvnorm), ranks by gev_sort_pairs_f64
//   :2286-2326  couples, inbreeding k_am_couples
//   :2328-2355  offspring numbers   k_pois_next / k_pois_double / k_pois_start ('p'), k_shuf_* + k_am_fixed_plus ('f')
//   :2394-2493  parent list         k_am_offspring_count + scan + k_am_expand
//
// Device log() (template, Marsaglia polar method) may differ from glibc's in the last bit; that can change a couple only where two
// template values lie within a few ulp of each other (the same statement as the GEF / selection calls' 1e-12).
#pragma once

#define AM_B 512                       // individuals per chunk of the marriage-draw chain
#define AM_SENT 0xffffffffu            // "no value" in the window / Poisson tables
enum { AMS_NM = 0, AMS_NF = 1, AMS_FLAGS = 2, AMS_NDIRECT = 3, AMS_NINB = 4, AMS_NACC = 5, AMS_WORDS = 8 };
enum { AMF_TPL_SHORT = 1, AMF_POIS_SHORT = 2 };

// one individual of the marriage-draw walk: consumes the selection draw and (for a marriageable male or female) the --MM draw at
// stream position d + i; returns the flag byte (1 male / 2 female / 0 not marriageable, +4 = second spouse) and advances x and d
__device__ __forceinline__ u32 am_step(u32& x, u32& d, double svf, bool has_svf, u32 s, double mm)
{
    const u32 x1 = mulmod31(x, 16807u), x2 = mulmod31(x1, 16807u);
    x = x2;
    const bool pass = has_svf ? (canonical_f64(x1, x2) < svf) : true;     // NaN: false; svf == NULL: every value is 1 (r < 1 always)
    if (!pass || (s != 1u && s != 2u)) return 0u;
    const u32 y1 = mulmod31(x, 16807u), y2 = mulmod31(y1, 16807u);
    x = y2; d++;
    return s | (canonical_f64(y1, y2) < mm ? 4u : 0u);
}

// chunk c: E = sum of P(pass) over its marriageable individuals, V = sum of P(1-P) (double2 per chunk)
__global__ void __launch_bounds__(256) k_am_chunk_stats(const uint8_t* __restrict__ sex, const u32* __restrict__ logical, const double* __restrict__ svf,
                                                       size_t n_h, double2* __restrict__ stats)
{
    __shared__ double le[256], lv[256];
    const size_t i0 = (size_t)blockIdx.x * AM_B;
    double e = 0, v = 0;
    for (u32 q = threadIdx.x; q < AM_B; q += 256) {
        const size_t i = i0 + q;
        if (i >= n_h) break;
        const u32 s = sex[logical ? logical[i] : i];
        if (s != 1u && s != 2u) continue;
        double p = svf ? svf[i] : 1.0;
        p = p != p ? 0.0 : fmin(fmax(p, 0.0), 1.0);
        e += p; v += p * (1.0 - p);
    }
    le[threadIdx.x] = e; lv[threadIdx.x] = v;
    __syncthreads();
    for (u32 st = 128; st; st >>= 1) {
        if (threadIdx.x < st) { le[threadIdx.x] += le[threadIdx.x + st]; lv[threadIdx.x] += lv[threadIdx.x + st]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) stats[blockIdx.x] = make_double2(le[0], lv[0]);
}
// window of start offsets of every chunk: [lo, lo + w), centred on the expected offset, half-width alpha * sd + kmin, w <= wcap
__global__ void __launch_bounds__(64) k_am_windows(const double2* __restrict__ stats, u32 n_chunks, double alpha, u32 kmin, u32 wcap,
                                                  u32* __restrict__ lo, u32* __restrict__ w)
{
    if (threadIdx.x || blockIdx.x) return;
    double E = 0, V = 0;
    for (u32 c = 0; c < n_chunks; c++) {
        const double K = ceil(alpha * sqrt(V)) + (double)kmin;
        const double l = fmax(floor(E) - K, 0.0);
        const double hi = fmin(floor(E) + K, (double)c * AM_B);          // d <= number of individuals in front
        lo[c] = (u32)l;
        w[c] = hi < l ? 0u : (u32)fmin(hi - l + 1.0, (double)wcap);
        E += stats[c].x; V += stats[c].y;
    }
}
// one lane per start offset of the chunk's window: walk the chunk, ends[c * wcap + lane] = offset behind it
__global__ void __launch_bounds__(256) k_am_walk(const uint8_t* __restrict__ sex, const u32* __restrict__ logical, const double* __restrict__ svf, size_t n_h,
                                                 u32 x0, double mm, const u32* __restrict__ lo, const u32* __restrict__ w, u32 wcap, u32* __restrict__ ends)
{
    __shared__ double ls[AM_B];
    __shared__ uint8_t lx[AM_B];
    const u32 c = blockIdx.x;
    const size_t i0 = (size_t)c * AM_B;
    const u32 nb = (u32)min((size_t)AM_B, n_h - i0);
    for (u32 q = threadIdx.x; q < nb; q += 256) { ls[q] = svf ? svf[i0 + q] : 1.0; lx[q] = sex[logical ? logical[i0 + q] : i0 + q]; }
    __syncthreads();
    const u32 lane = blockIdx.y * 256 + threadIdx.x;
    if (lane >= w[c]) return;
    u32 d = lo[c] + lane;
    u32 x = mulmod31(powmod31(16807u, 2 * ((u64)i0 + d)), x0);            // engine state in front of draw i0 + d
    for (u32 q = 0; q < nb; q++) (void)am_step(x, d, ls[q], svf != nullptr, lx[q], mm);
    ends[(size_t)c * wcap + lane] = d;
}
// the chain over the chunks from offset 0: start[c] = true offset in front of chunk c.  A start outside the chunk's window is walked
// directly (counted in stat[AMS_NDIRECT]); stat[AMS_NACC] = the offset behind the last chunk.
__global__ void __launch_bounds__(64) k_am_chain(const uint8_t* __restrict__ sex, const u32* __restrict__ logical, const double* __restrict__ svf, size_t n_h,
                                                 u32 x0, double mm, u32 n_chunks, const u32* __restrict__ lo, const u32* __restrict__ w, u32 wcap,
                                                 const u32* __restrict__ ends, u32* __restrict__ start, u32* __restrict__ stat)
{
    if (threadIdx.x || blockIdx.x) return;
    u32 d = 0, n_direct = 0;
    for (u32 c = 0; c < n_chunks; c++) {
        start[c] = d;
        const u32 l = lo[c];
        if (d >= l && d - l < w[c]) { d = ends[(size_t)c * wcap + (d - l)]; continue; }
        n_direct++;
        const size_t i0 = (size_t)c * AM_B, i1 = min(i0 + AM_B, n_h);
        u32 x = mulmod31(powmod31(16807u, 2 * ((u64)i0 + d)), x0);
        for (size_t i = i0; i < i1; i++) (void)am_step(x, d, svf ? svf[i] : 1.0, svf != nullptr, sex[logical ? logical[i] : i], mm);
    }
    stat[AMS_NDIRECT] = n_direct; stat[AMS_NACC] = d;
}
// chunk c walked once from its true start: cm[i] / cf[i] = entries of individual i in the male / female list (0, 1 or 2)
__global__ void __launch_bounds__(256) k_am_flags(const uint8_t* __restrict__ sex, const u32* __restrict__ logical, const double* __restrict__ svf, size_t n_h,
                                                  u32 x0, double mm, const u32* __restrict__ start, u32* __restrict__ cm, u32* __restrict__ cf)
{
    __shared__ double ls[AM_B];
    __shared__ uint8_t lx[AM_B], lf[AM_B];
    const u32 c = blockIdx.x;
    const size_t i0 = (size_t)c * AM_B;
    const u32 nb = (u32)min((size_t)AM_B, n_h - i0);
    for (u32 q = threadIdx.x; q < nb; q += 256) { ls[q] = svf ? svf[i0 + q] : 1.0; lx[q] = sex[logical ? logical[i0 + q] : i0 + q]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 d = start[c];
        u32 x = mulmod31(powmod31(16807u, 2 * ((u64)i0 + d)), x0);
        for (u32 q = 0; q < nb; q++) lf[q] = (uint8_t)am_step(x, d, ls[q], svf != nullptr, lx[q], mm);
    }
    __syncthreads();
    for (u32 q = threadIdx.x; q < nb; q += 256) {
        const u32 f = lf[q], k = (f & 4u) ? 2u : 1u;
        cm[i0 + q] = (f & 3u) == 1u ? k : 0u;
        cf[i0 + q] = (f & 3u) == 2u ? k : 0u;
    }
}
// pos_male_marriageable / pos_female_marriageable (:2185-2200) in individual order, a second spouse next to its first entry
__global__ void __launch_bounds__(256) k_am_compact(const u32* __restrict__ cm, const u32* __restrict__ cf, const u32* __restrict__ om, const u32* __restrict__ of,
                                                    size_t n_h, u32* __restrict__ males, u32* __restrict__ females, u32* __restrict__ stat)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { stat[AMS_NM] = om[n_h]; stat[AMS_NF] = of[n_h]; }
    if (i >= n_h) return;
    for (u32 k = 0; k < cm[i]; k++) males[om[i] + k] = (u32)i;
    for (u32 k = 0; k < cf[i]; k++) females[of[i] + k] = (u32)i;
}

// ---- glibc rand() after srand(seed): out[k] = the (k+1)-th rand() value, k < n (one wave, GlibcWave of rng_device.h) -------------
__global__ void __launch_bounds__(64) k_glibc_stream(const GevRngTables* __restrict__ T, u32 seed, size_t n, u32* __restrict__ out)
{
    GlibcWave g;
    g.seed(T, seed);
    const u32 lane = threadIdx.x;
    for (size_t b = 0; b * 64 < n; b++) {
        if (b) g.next_block(T);
        const size_t k = b * 64 + lane;
        if (k < n) out[k] = g.x >> 1;
    }
}
// ---- std::random_shuffle(first, first + m) on rand() values R (:2232-2246, :2346): for i = 1..m-1 swap(i, J_i), J_i = R[i-1] % (i+1).
// The element that ends at position p is found without replaying the swaps: undoing them from the last, position p is first touched
// by the LAST swap i > p with J_i == p (the element came from i, and nothing later moves i again); if there is none, swap p moves it
// to J_p and the question repeats for J_p with only the swaps before p left.  tgt lists every i with J_i = t != i (CSR by t).
__global__ void __launch_bounds__(256) k_shuf_count(const u32* __restrict__ R, size_t m, u32* __restrict__ cnt)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x + 1;
    if (i >= m) return;
    const u32 j = R[i - 1] % (u32)(i + 1);
    if (j != (u32)i) atomicAdd(cnt + j, 1u);
}
__global__ void __launch_bounds__(256) k_shuf_fill(const u32* __restrict__ R, size_t m, const u32* __restrict__ off, u32* __restrict__ fill, u32* __restrict__ tgt)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x + 1;
    if (i >= m) return;
    const u32 j = R[i - 1] % (u32)(i + 1);
    if (j != (u32)i) tgt[off[j] + atomicAdd(fill + j, 1u)] = (u32)i;
}
// src[p - p0] = original position of the element at final position p, p in [p0, p1)
__global__ void __launch_bounds__(256) k_shuf_trace(const u32* __restrict__ R, size_t m, const u32* __restrict__ off, const u32* __restrict__ tgt,
                                                    size_t p0, size_t p1, u32* __restrict__ src)
{
    const size_t p = p0 + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= p1) return;
    u32 cur = (u32)p, bound = (u32)m;
    for (;;) {
        u32 best = 0; bool found = false;
        for (u32 q = off[cur]; q < off[cur + 1]; q++) { const u32 i = tgt[q]; if (i < bound && (!found || i > best)) { best = i; found = true; } }
        if (found) { cur = best; break; }
        if (cur == 0) break;
        const u32 j = R[cur - 1] % (cur + 1);
        if (j == cur) break;
        bound = cur; cur = j;
    }
    src[p - p0] = cur;
}
__global__ void __launch_bounds__(256) k_gather_u32(const u32* __restrict__ in, const u32* __restrict__ idx, size_t n, u32* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[idx[i]];
}

// ---- ras_mvnorm (:2268, RasRandomNumber.cpp:15-51): Marsaglia polar pairs on default_random_engine(seed2), drawn by the skeleton
// of gev_normal.h; row i of z = the i-th accepted pair (y*mult, x*mult); t1 / t2 = z * chol without FMA
__global__ void __launch_bounds__(256) k_tpl_count(u32 x0, u64 n_cand, u32* __restrict__ blk)
{
    __shared__ u32 lds[8];
    polar_count_block(x0, n_cand, blk, lds);
}
__global__ void __launch_bounds__(256) k_tpl_emit(u32 x0, u64 n_cand, u64 n2, const u32* __restrict__ blk, double u01, double u11,
                                                  double* __restrict__ t1, double* __restrict__ t2, u32* __restrict__ stat)
{
    __shared__ u32 lds[8];
    polar_emit_block(x0, n_cand, n2, gridDim.x, blk, lds, stat + AMS_FLAGS, (u32)AMF_TPL_SHORT, [&](u64 k, double xx, double yy, double r2, u32) {
        const double mult = polar_mult(r2);
        const double z0 = __dmul_rn(yy, mult), z1 = __dmul_rn(xx, mult);
        t1[k] = __dadd_rn(__dadd_rn(0.0, __dmul_rn(z0, 1.0)), __dmul_rn(z1, 0.0));
        t2[k] = __dadd_rn(__dadd_rn(0.0, __dmul_rn(z0, u01)), __dmul_rn(z1, u11));
    });
}

// ---- couples (:2286-2326): couple i = (males sorted by mv at rank_t1[i], females sorted at rank_t2[i]); position p of the stable sort
// of t1 holds index i1[p] = the couple whose rank is p.  With avoid_inbreeding the eight-way test on the pedigree ids [n][5] =
// (ID_Father, ID_Fathers_Father, ID_Fathers_Mother, ID_Mothers_Father, ID_Mothers_Mother).
__global__ void __launch_bounds__(256) k_am_couples(const u32* __restrict__ i1, const u32* __restrict__ i2, const u32* __restrict__ ms, const u32* __restrict__ fs,
                                                    size_t n2, u32* __restrict__ pm, u32* __restrict__ pf)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n2) return;
    pm[i1[p]] = ms[p];
    pf[i2[p]] = fs[p];
}
__global__ void __launch_bounds__(256) k_am_inbreed(const u32* __restrict__ pm, const u32* __restrict__ pf, size_t n2, const int64_t* __restrict__ ped,
                                                    u32* __restrict__ inb, u32* __restrict__ stat)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n2) return;
    u32 v = 0;
    if (ped) {
        const int64_t* a = ped + (size_t)pm[i] * 5;
        const int64_t* b = ped + (size_t)pf[i] * 5;
        const bool sib = a[0] == b[0];
        const bool cousin = a[1] == b[1] || a[1] == b[3] || a[3] == b[1] || a[3] == b[3] ||
                            a[2] == b[2] || a[2] == b[4] || a[4] == b[2] || a[4] == b[4];
        v = (sib || cousin) ? 1u : 0u;
        if (v) atomicAdd(stat + AMS_NINB, 1u);
    }
    inb[i] = v;
}

// ---- ras_rpois (:2330, RasRandomNumber.cpp:56-66): poisson_distribution, product of uniforms (mean < 12) on default_random_engine(seed3).
// A couple whose draws start at stream position s ends at nxt[s] (the first position whose running product is <= thr, plus one);
// couple k starts at nxt^k(0), found by pointer doubling.  nxt[s] = AM_SENT when the S draws end before the product does.
__global__ void __launch_bounds__(256) k_pois_next(u32 x0, u64 S, double thr, u32* __restrict__ nxt)
{
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s > S) return;
    u32 r = AM_SENT;
    if (s < S) {
        u32 x = mulmod31(powmod31(16807u, 2 * s), x0);
        double prod = 1.0;
        for (u64 k = s; k < S; k++) {
            const u32 x1 = mulmod31(x, 16807u), x2 = mulmod31(x1, 16807u);
            x = x2;
            prod = __dmul_rn(prod, canonical_f64(x1, x2));
            if (!(prod > thr)) { r = (u32)(k + 1); break; }
        }
    }
    nxt[s] = r;
}
__global__ void __launch_bounds__(256) k_pois_double(const u32* __restrict__ a, u64 S, u32* __restrict__ b)
{
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s > S) return;
    const u32 v = a[s];
    b[s] = v == AM_SENT ? AM_SENT : a[v];
}
// tabs = levels 0..L-1 (level j = nxt^(2^j)), each S+1 words
__global__ void __launch_bounds__(256) k_pois_start(const u32* __restrict__ tabs, u64 S, u32 L, u64 n2, int32_t* __restrict__ num, u32* __restrict__ stat)
{
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n2) return;
    u32 s = 0;
    for (u32 j = 0; j < L && s != AM_SENT; j++)
        if ((k >> j) & 1u) s = tabs[(size_t)j * (S + 1) + s];
    const u32 e = s == AM_SENT ? AM_SENT : tabs[s];
    if (e == AM_SENT) { atomicOr(stat + AMS_FLAGS, (u32)AMF_POIS_SHORT); num[k] = 0; return; }
    num[k] = (int32_t)(e - s - 1);
}
__global__ void __launch_bounds__(256) k_am_fill_i32(int32_t* __restrict__ a, size_t n, int32_t v)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = v;
}
// 'f' (:2340-2352): the first `remain` couples of the shuffled pos_couple_can_marry get one more child (idx: their original positions)
__global__ void __launch_bounds__(256) k_am_fixed_plus(const u32* __restrict__ idx, size_t remain, int32_t* __restrict__ num)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < remain) num[idx[i]] += 1;
}

// ---- the offspring list (:2433-2443): couple order, num_offspring children each, inbred couples none --------------------------
__global__ void __launch_bounds__(256) k_am_offspring_count(const int32_t* __restrict__ num, const u32* __restrict__ inb, size_t n2, u32* __restrict__ cnt)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n2) cnt[i] = inb[i] ? 0u : (u32)max(num[i], 0);
}
__global__ void __launch_bounds__(256) k_am_expand(const u32* __restrict__ pm, const u32* __restrict__ pf, const int32_t* __restrict__ num, const u32* __restrict__ inb,
                                                   const u32* __restrict__ off, size_t n2, const u32* __restrict__ logical,
                                                   u32* __restrict__ father, u32* __restrict__ mother, gev_couple* __restrict__ couples)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n2) return;
    const u32 m = pm[i], f = pf[i];
    if (couples) { couples[i].pos_male = m; couples[i].pos_female = f; couples[i].inbreed = (int32_t)inb[i]; couples[i].num_offspring = num[i]; }
    if (father) {
        const u32 rm = logical ? logical[m] : m, rf = logical ? logical[f] : f;
        for (u32 q = off[i]; q < off[i + 1]; q++) { father[q] = rm; mother[q] = rf; }
    }
}
