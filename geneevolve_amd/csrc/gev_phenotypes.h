// gev_phenotypes.h -- Simulation::ras_scale_AD_compute_GEF (reference src/Simulation.cpp:3075-3206) for every phenotype of a population
// from state the library holds (gev_generation_phenotypes): the family effect of Simulation::reproduce (:2417-2429, :2481-2484) and of
// generation 0 (:3053-3066), the noise and generation-0 parental streams, the parental effect gathered from the saved record BY ID
// (:3118-3131), var(e), the scaling, and CommFunc::var of the seven components.  Nothing here reads a host value that depends on the
// device: seeds, stream offsets, means and variances are device words.  Included by gev_library.hip behind gev_pedigree.h; built
// with -ffp-contract=off like the rest of the library.
#pragma once
#include "gev_kernels.h"
#include "gev_select.h"
#include "gev_pedigree.h"

enum { PH_A = 0, PH_D, PH_G, PH_C, PH_E, PH_F, PH_P, PH_COMP };              // planes of a phenotype's components, n doubles each
enum { PHF_CAND_SHORT = 256 /* a normal stream ran out of candidate pairs: run again with more */,
       PHF_ID_RANGE = 512 /* a parent id at or beyond the saved record's length (undefined behaviour in the reference) */ };
enum { PHR_STATE = 0, PHR_FLAGS = 1, PHR_NBAD = 2, PHR_SEEDS = 4 };          // result words; seeds: one per phenotype with vc > 0 (generation 0), then one per phenotype

// one std::normal_distribution stream: n values of N(0, sd) on default_random_engine(seed + seed_add), the first candidate pair being
// pair number starts[start_idx] of the engine (a fresh distribution on an engine another one has used: reproduce's common-effect loop)
struct NrmStream {
    int seed_idx;            // >= 0: seed = seeds[seed_idx] (a ras_glob_seed() value drawn on the device); < 0: seed_val
    u32 seed_val, seed_add;
    int start_idx, next_idx; // >= 0: first pair = starts[start_idx]; starts[next_idx] = the pair behind the last one consumed
    u32 n_blocks, blk_off;   // this stream's blocks of the grid and its slice of the block counts
    u32 pad;
    u64 n, n_cand;
    double sd;
    double* out;
};
#define NRM_PER_THREAD 8
#define NRM_CHUNK (256 * NRM_PER_THREAD)

__device__ __forceinline__ u32 nrm_state(const NrmStream& s, const u32* seeds, const u32* starts, u64 m0, u64& first_pair)
{
    const u32 seed = (s.seed_idx >= 0 ? seeds[s.seed_idx] : s.seed_val) + s.seed_add;
    first_pair = s.start_idx >= 0 ? starts[s.start_idx] : 0;
    return mulmod31(powmod31(16807u, 4 * (first_pair + m0)), minstd_seed(seed));
}
__global__ void __launch_bounds__(256) k_nrm_count(const NrmStream* __restrict__ streams, const u32* __restrict__ seeds, const u32* __restrict__ starts, u32* __restrict__ blk)
{
    __shared__ u32 lds[8];
    const NrmStream s = streams[blockIdx.y];
    if (blockIdx.x >= s.n_blocks) return;
    const u64 m0 = (u64)blockIdx.x * NRM_CHUNK + (u64)threadIdx.x * NRM_PER_THREAD;
    u32 cnt = 0;
    if (m0 < s.n_cand) {
        u64 fp;
        u32 x = nrm_state(s, seeds, starts, m0, fp);
        for (int q = 0; q < NRM_PER_THREAD && m0 + q < s.n_cand; q++) { double a, b, r; cnt += tpl_candidate(x, a, b, r) ? 1u : 0u; }
    }
    const u32 tot = block_sum_256(cnt, lds);
    if (threadIdx.x == 0) blk[s.blk_off + blockIdx.x] = tot;
}
__global__ void __launch_bounds__(256) k_nrm_emit(const NrmStream* __restrict__ streams, const u32* __restrict__ seeds, u32* __restrict__ starts, const u32* __restrict__ blk,
                                                  u32* __restrict__ flags)
{
    __shared__ u32 lds[8];
    const NrmStream s = streams[blockIdx.y];
    if (blockIdx.x >= s.n_blocks) return;
    u32 part = 0;
    for (u32 b = threadIdx.x; b < blockIdx.x; b += 256) part += blk[s.blk_off + b];
    const u32 before_blocks = block_sum_256(part, lds);
    const u64 m0 = (u64)blockIdx.x * NRM_CHUNK + (u64)threadIdx.x * NRM_PER_THREAD;
    const u64 pairs = (s.n + 1) / 2;                          // accepted pairs the n values consume (the last one's second value is dropped when n is odd)
    u32 acc = 0, x = 0;
    u64 fp = 0;
    if (m0 < s.n_cand) {
        x = nrm_state(s, seeds, starts, m0, fp);
        u32 y = x;
        for (int q = 0; q < NRM_PER_THREAD && m0 + q < s.n_cand; q++) { double a, b, r; acc |= (tpl_candidate(y, a, b, r) ? 1u : 0u) << q; }
    }
    u32 tot;
    const u32 before = before_blocks + block_exclusive_scan_256((u32)__popc(acc), lds, tot);
    if (blockIdx.x == s.n_blocks - 1 && threadIdx.x == 255 && (u64)before + __popc(acc) < pairs) atomicOr(flags, (u32)PHF_CAND_SHORT);
    if (m0 >= s.n_cand) return;
    u64 k = before;
    for (int q = 0; q < NRM_PER_THREAD && m0 + q < s.n_cand; q++) {
        double xx, yy, r2;
        const bool ok = tpl_candidate(x, xx, yy, r2);
        if (!ok) continue;
        if (k < pairs) {
            const double mult = sqrt(-2 * log(r2) / r2);
            s.out[2 * k] = yy * mult * s.sd + 0.0;                                   // ret * stddev + mean
            if (2 * k + 1 < s.n) s.out[2 * k + 1] = xx * mult * s.sd + 0.0;
            if (k == pairs - 1 && s.next_idx >= 0) starts[s.next_idx] = (u32)(fp + m0 + q + 1);
        }
        k++;
    }
}

// CommFunc::mean / CommFunc::var (src/CommFunc.cpp:38-68) of several vectors at once: vector v = base + v * vec_stride, element i at
// [i * elem_stride]; stats[v] = {mean, var (n-1; 0 for n <= 1)}.  pass 0 sums x, pass 1 sums (x - mean)^2 with the mean of pass 0.
// The sums are formed as k_sum_partial / k_sum_final form them (gev_scale_ad_compute_gef): min(ceil(n/256), 256) blocks, then one.
__global__ void __launch_bounds__(256) k_ph_var_partial(const double* __restrict__ base, size_t vec_stride, size_t elem_stride, size_t n, const double* __restrict__ stats,
                                                        int pass, double* __restrict__ partial)
{
    __shared__ double s[256];
    const double* x = base + blockIdx.y * vec_stride;
    const double mu = pass ? stats[2 * blockIdx.y] : 0.0;
    double acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { const double v = x[i * elem_stride] - mu; acc += pass ? v * v : v; }
    s[threadIdx.x] = acc; __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) partial[blockIdx.y * 256 + blockIdx.x] = s[0];
}
__global__ void __launch_bounds__(256) k_ph_var_final(const double* __restrict__ partial, int nb, size_t n, int pass, double* __restrict__ stats)
{
    __shared__ double s[256];
    s[threadIdx.x] = (int)threadIdx.x < nb ? partial[blockIdx.x * 256 + threadIdx.x] : 0.0; __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) {
        if (pass == 0) stats[2 * blockIdx.x] = s[0] / (double)n;
        else stats[2 * blockIdx.x + 1] = n <= 1 ? 0.0 : s[0] / (double)(n - 1);
    }
}

// what the apply needs per phenotype (a device table: no limit on the number of phenotypes)
struct PhTask {
    double s_a, s_d, ve, vf, beta;
    int has_c;               // vc > 0
    int c_by_couple;         // generation > 0: C = cval[couple of the child]; generation 0: the C plane already holds the stream
    int f_gather;            // generation > 0 and vf > 0: F = beta * (prev[ID_Father] + prev[ID_Mother]); else the F plane holds the generation-0 stream (vf > 0)
    int prev_plane;          // 0: the saved record's phen (vt_type 1), 1: its parental_effect (vt_type 2), < 0: neither (0 + 0)
};
// :3104-3133 and :3174-3203 for all phenotypes: grid (ceil(n / 256), nphen).  comp = [nphen][PH_COMP][n]; raw a / d = [n][nphen];
// e_raw = [nphen][n]; cval = [nphen][cval_stride]; prev = [nphen][2][prev_n]; ids planes by physical row (positions are rows here)
__global__ void __launch_bounds__(256) k_ph_apply(const PhTask* __restrict__ tasks, const double* __restrict__ a, const double* __restrict__ d, size_t n, u32 nphen,
                                                  const double* __restrict__ e_raw, const double* __restrict__ e_stats, const double* __restrict__ cval, size_t cval_stride,
                                                  const int64_t* __restrict__ ids, size_t ids_stride, const u32* __restrict__ cidx,
                                                  const double* __restrict__ prev, size_t prev_n, double* __restrict__ comp, double* __restrict__ keep, u32* __restrict__ res)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 p = blockIdx.y;
    const PhTask t = tasks[p];
    double* o = comp + (size_t)p * PH_COMP * n;
    double s_ev = 0;
    if (t.ve > 0) s_ev = sqrt(e_stats[2 * p + 1] / t.ve);
    const double en = s_ev > 0 ? e_raw[(size_t)p * n + i] / s_ev : 0;
    const double ad = a[i * nphen + p] / t.s_a;
    const double dm = t.s_d > 0 ? d[i * nphen + p] / t.s_d : 0;
    double pe = 0;
    if (t.vf > 0) {
        if (t.f_gather) {
            double ff = 0, fm = 0;
            if (t.prev_plane >= 0) {
                const int64_t idf = ids[PED_FATHER * ids_stride + i], idm = ids[PED_MOTHER * ids_stride + i];
                if (idf < 0 || idm < 0 || (u64)idf >= prev_n || (u64)idm >= prev_n) { atomicOr(res + PHR_FLAGS, (u32)PHF_ID_RANGE); atomicAdd(res + PHR_NBAD, 1u); }
                else { const double* pv = prev + ((size_t)p * 2 + t.prev_plane) * prev_n; ff = pv[idf]; fm = pv[idm]; }
            }
            pe = t.beta * (ff + fm);
        } else pe = o[PH_F * n + i];
    }
    double cs = 0.0;
    if (t.has_c) cs = t.c_by_couple ? cval[(size_t)p * cval_stride + cidx[i]] : o[PH_C * n + i];
    o[PH_A * n + i] = ad; o[PH_D * n + i] = dm; o[PH_G * n + i] = ad + dm; o[PH_C * n + i] = cs; o[PH_E * n + i] = en; o[PH_F * n + i] = pe;
    const double ph = ad + dm + cs + en + pe;
    o[PH_P * n + i] = ph; keep[i * nphen + p] = ph;
}
// the previous-generation record (ras_save_human_info_to_Pop_info_prev_gen, :3211-3236): phen (+ the --gamma constant of :3292) and
// parental_effect of the current individuals in position order, rec = [nphen][2][n]
__global__ void __launch_bounds__(256) k_ph_save_prev(const double* __restrict__ comp, size_t n, const double* __restrict__ shift, double* __restrict__ rec)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 p = blockIdx.y;
    const double* o = comp + (size_t)p * PH_COMP * n;
    rec[((size_t)p * 2 + 0) * n + i] = shift ? o[PH_P * n + i] + shift[p] : o[PH_P * n + i];
    rec[((size_t)p * 2 + 1) * n + i] = o[PH_F * n + i];
}
