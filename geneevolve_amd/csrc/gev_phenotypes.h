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
enum { PHF_CAND_SHORT = NRM_CAND_SHORT /* a normal stream ran out of candidate pairs: run again with more */,
       PHF_ID_RANGE = 512 /* a parent id at or beyond the saved record's length (undefined behaviour in the reference) */ };
enum { PHR_STATE = 0, PHR_FLAGS = 1, PHR_NBAD = 2, PHR_SEEDS = 4 };          // result words; seeds: one per phenotype with vc > 0 (generation 0), then one per phenotype

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
    const GefValues v = gef_scale(a[i * nphen + p], d[i * nphen + p], t.s_a, t.s_d, e_raw[(size_t)p * n + i], e_stats[2 * p + 1], t.ve, cs, pe);
    o[PH_A * n + i] = v.a; o[PH_D * n + i] = v.d; o[PH_G * n + i] = v.g; o[PH_C * n + i] = cs; o[PH_E * n + i] = v.e; o[PH_F * n + i] = pe;
    o[PH_P * n + i] = v.p; keep[i * nphen + p] = v.p;
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
