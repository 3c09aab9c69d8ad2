// gev_normal.h -- std::normal_distribution<double> on std::minstd_rand0 (libstdc++ bits/random.tcc:1802-1835: Marsaglia polar method
// with rejection) on the device (gfx950, wave64), and CommFunc::mean / CommFunc::var of what it draws.  Included by gev_kernels.h
// behind gev_mate.h.  Every caller draws through the one skeleton below, so their streams agree bit for bit by construction:
//
//   ras_mvnorm of assort_mate (the template)               k_tpl_count / k_tpl_emit   (gev_assort.h)
//   noise, family and parental streams of the phenotypes   k_nrm_count / k_nrm_emit   (gev_generation_phenotypes, gev_scale_ad_compute_gef)
//
// Candidate pair m consumes engine outputs 4m+1 .. 4m+4 (two generate_canonical draws, computed in FP64 as libstdc++ does, no
// contraction); the k-th ACCEPTED pair yields the normals 2k (= y * mult) and 2k+1 (= x * mult).  Engine output number j is
// 16807^j * state (mod 2^31 - 1), so every candidate is evaluated independently by jump-ahead: pass 1 counts the accepted pairs of
// every block of POLAR_CHUNK candidates, pass 2 sums the counts of the blocks in front, ranks its own candidates with a block scan
// and hands the accepted ones to the caller's store.  log() is the device libm (<= 1 ulp from glibc's).
#pragma once

#define POLAR_PER_THREAD 8
#define POLAR_CHUNK (256 * POLAR_PER_THREAD)  // candidate pairs per block

__device__ __forceinline__ bool polar_candidate(u32& x, double& xx, double& yy, double& r2)
{
    const u32 x1 = mulmod31(x, 16807u), x2 = mulmod31(x1, 16807u), x3 = mulmod31(x2, 16807u), x4 = mulmod31(x3, 16807u);
    x = x4;
    xx = __dadd_rn(__dmul_rn(2.0, canonical_f64(x1, x2)), -1.0);
    yy = __dadd_rn(__dmul_rn(2.0, canonical_f64(x3, x4)), -1.0);
    r2 = __dadd_rn(__dmul_rn(xx, xx), __dmul_rn(yy, yy));
    return !(r2 > 1.0 || r2 == 0.0);
}
__device__ __forceinline__ double polar_mult(double r2) { return sqrt(-2 * log(r2) / r2); }

// pass 1: blk[blockIdx.x] = accepted pairs among this block's candidates; x_first = the engine state in front of candidate pair 0
__device__ __forceinline__ void polar_count_block(u32 x_first, u64 n_cand, u32* __restrict__ blk, u32* lds)
{
    const u64 m0 = (u64)blockIdx.x * POLAR_CHUNK + (u64)threadIdx.x * POLAR_PER_THREAD;
    u32 cnt = 0;
    if (m0 < n_cand) {
        u32 x = mulmod31(powmod31(16807u, 4 * m0), x_first);
        for (int q = 0; q < POLAR_PER_THREAD && m0 + q < n_cand; q++) { double a, b, r; cnt += polar_candidate(x, a, b, r) ? 1u : 0u; }
    }
    const u32 tot = block_sum_256(cnt, lds);
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}
// pass 2: emit(k, xx, yy, r2, m) for the k-th accepted pair (k < pairs), m = its candidate index (32 bits, like the counts and the
// stream offsets).  The candidates are evaluated twice: the mask for the ranks first, then the values.  The last thread of the
// stream's last block (n_blocks of them) sets *short_flag |= flag_bit when the n_cand candidates hold fewer than `pairs` accepted
// ones: the caller runs again with more.
template <class Emit>
__device__ __forceinline__ void polar_emit_block(u32 x_first, u64 n_cand, u64 pairs, u32 n_blocks, const u32* __restrict__ blk, u32* lds, u32* short_flag, u32 flag_bit, Emit&& emit)
{
    u32 part = 0;
    for (u32 b = threadIdx.x; b < blockIdx.x; b += 256) part += blk[b];
    const u32 before_blocks = block_sum_256(part, lds);
    const u64 m0 = (u64)blockIdx.x * POLAR_CHUNK + (u64)threadIdx.x * POLAR_PER_THREAD;
    u32 acc = 0, x = 0;
    if (m0 < n_cand) {
        x = mulmod31(powmod31(16807u, 4 * m0), x_first);
        u32 y = x;
        for (int q = 0; q < POLAR_PER_THREAD && m0 + q < n_cand; q++) { double a, b, r; acc |= (polar_candidate(y, a, b, r) ? 1u : 0u) << q; }
    }
    u32 tot;
    const u32 before = before_blocks + block_exclusive_scan_256((u32)__popc(acc), lds, tot);
    if (blockIdx.x == n_blocks - 1 && threadIdx.x == 255 && (u64)before + __popc(acc) < pairs) atomicOr(short_flag, flag_bit);
    if (m0 >= n_cand) return;
    u64 k = before;
    for (int q = 0; q < POLAR_PER_THREAD && m0 + q < n_cand; q++) {
        double xx, yy, r2;
        const bool ok = polar_candidate(x, xx, yy, r2);
        if (!ok) continue;
        if (k < pairs) emit(k, xx, yy, r2, (u32)m0 + (u32)q);
        k++;
    }
}

// ---- batched streams: one grid row per stream, seeds and start offsets as device words ---------------------------------------------
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
enum { NRM_CAND_SHORT = 256 };  // the flag bit of a stream that ran out of candidate pairs (PHF_CAND_SHORT of gev_phenotypes.h)

__device__ __forceinline__ u32 nrm_first(const NrmStream& s, const u32* seeds, const u32* starts, u64& first_pair)
{
    const u32 seed = (s.seed_idx >= 0 ? seeds[s.seed_idx] : s.seed_val) + s.seed_add;
    first_pair = s.start_idx >= 0 ? starts[s.start_idx] : 0;
    return mulmod31(powmod31(16807u, 4 * first_pair), minstd_seed(seed));
}
__global__ void __launch_bounds__(256) k_nrm_count(const NrmStream* __restrict__ streams, const u32* __restrict__ seeds, const u32* __restrict__ starts, u32* __restrict__ blk)
{
    __shared__ u32 lds[8];
    const NrmStream s = streams[blockIdx.y];
    if (blockIdx.x >= s.n_blocks) return;
    u64 fp;
    polar_count_block(nrm_first(s, seeds, starts, fp), s.n_cand, blk + s.blk_off, lds);
}
__global__ void __launch_bounds__(256) k_nrm_emit(const NrmStream* __restrict__ streams, const u32* __restrict__ seeds, u32* __restrict__ starts, const u32* __restrict__ blk,
                                                  u32* __restrict__ flags)
{
    __shared__ u32 lds[8];
    const NrmStream s = streams[blockIdx.y];
    if (blockIdx.x >= s.n_blocks) return;
    u64 fp;
    const u32 x_first = nrm_first(s, seeds, starts, fp);
    const u64 pairs = (s.n + 1) / 2;                          // accepted pairs the n values consume (the last one's second value is dropped when n is odd)
    polar_emit_block(x_first, s.n_cand, pairs, s.n_blocks, blk + s.blk_off, lds, flags, (u32)NRM_CAND_SHORT, [&](u64 k, double xx, double yy, double r2, u32 m) {
        const double mult = polar_mult(r2);
        s.out[2 * k] = yy * mult * s.sd + 0.0;                                   // ret * stddev + mean
        if (2 * k + 1 < s.n) s.out[2 * k + 1] = xx * mult * s.sd + 0.0;
        if (k == pairs - 1 && s.next_idx >= 0) starts[s.next_idx] = (u32)fp + m + 1u;
    });
}

// ---- CommFunc::mean / CommFunc::var (src/CommFunc.cpp:38-68) of several vectors at once: vector v = base + v * vec_stride, element i
// at [i * elem_stride]; stats[v] = {mean, var (n-1; 0 for n <= 1)}.  pass 0 sums x, pass 1 sums (x - mean)^2 with the mean of pass 0.
// min(ceil(n/256), 256) blocks of grid-stride partial sums, then one block per vector: the one summation order of var(e), of the
// component variances and of the generation-0 selection statistics.
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
