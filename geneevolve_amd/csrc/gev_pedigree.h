// gev_pedigree.h -- the ID fields of reference `class Human` (src/Population.h:126-137) on the device (gev_set_track_pedigree).
//
// Seven planes of int64, one per field, `stride` rows apart: a wave's accesses to one field are contiguous.  Row = the
// individual's PHYSICAL row (what the father / mother arrays of a generation name); positions go through `logical` where the two differ.
#pragma once
#include "gev_kernels.h"

enum { PED_ID = 0, PED_FATHER, PED_MOTHER, PED_FF, PED_FM, PED_MF, PED_MM, PED_FIELDS };

// generation 0: every field = i (src/Simulation.cpp:3037-3043)
__global__ void __launch_bounds__(256) k_ped_gen0(int64_t* __restrict__ ids, size_t stride, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int f = 0; f < PED_FIELDS; f++) ids[f * stride + i] = (int64_t)i;
}
// a published generation (src/Simulation.cpp:2473-2479): child i of father row fa[i] and mother row mo[i]; ID = i_people.
// cidx_out[i] = the index of the child's couple in the generation's couples list (what hands it its family effect, :2481-2484):
// cidx_src[i] where the host listed it, else the couple whose slice of the offspring offsets ooff[0..n2] holds i, else i (one child each)
__global__ void __launch_bounds__(256) k_ped_offspring(const int64_t* __restrict__ src, size_t sstride, size_t n_src, const u32* __restrict__ fa,
                                                       const u32* __restrict__ mo, size_t n, int64_t* __restrict__ dst, size_t dstride,
                                                       const u32* __restrict__ cidx_src, const u32* __restrict__ ooff, u32 n2, u32* __restrict__ cidx_out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t f = fa[i], m = mo[i];
    const bool okf = f < n_src, okm = m < n_src;               // (the rows were range-checked where the couples were formed)
    dst[PED_ID * dstride + i] = (int64_t)i;
    dst[PED_FATHER * dstride + i] = okf ? src[PED_ID * sstride + f] : -1;
    dst[PED_FF * dstride + i] = okf ? src[PED_FATHER * sstride + f] : -1;
    dst[PED_FM * dstride + i] = okf ? src[PED_MOTHER * sstride + f] : -1;
    dst[PED_MOTHER * dstride + i] = okm ? src[PED_ID * sstride + m] : -1;
    dst[PED_MF * dstride + i] = okm ? src[PED_FATHER * sstride + m] : -1;
    dst[PED_MM * dstride + i] = okm ? src[PED_MOTHER * sstride + m] : -1;
    u32 k = (u32)i;
    if (cidx_src) k = cidx_src[i];
    else if (ooff) {                                           // last k with ooff[k] <= i (couples without children share an offset)
        u32 lo = 0, hi = n2;
        while (lo + 1 < hi) { const u32 mid = (lo + hi) >> 1; if (ooff[mid] <= (u32)i) lo = mid; else hi = mid; }
        k = lo;
    }
    cidx_out[i] = k;
}
// [n][7] records in position order for the host (gev_download_pedigree)
__global__ void __launch_bounds__(256) k_ped_records(const int64_t* __restrict__ src, size_t sstride, const u32* __restrict__ logical, size_t n,
                                                     int64_t* __restrict__ out)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * PED_FIELDS) return;
    const size_t i = t / PED_FIELDS, f = t - i * PED_FIELDS;
    out[t] = src[f * sstride + (logical ? logical[i] : i)];
}
// k_am_inbreed (gev_assort.h) on the device's own ids: the sibling / cousin test of avoid_inbreeding (src/Simulation.cpp:2306-2322)
__global__ void __launch_bounds__(256) k_am_inbreed_ids(const u32* __restrict__ pm, const u32* __restrict__ pf, size_t n2, const int64_t* __restrict__ ids,
                                                        size_t stride, const u32* __restrict__ logical, u32* __restrict__ inb, u32* __restrict__ stat)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n2) return;
    const size_t a = logical ? logical[pm[i]] : pm[i], b = logical ? logical[pf[i]] : pf[i];
    const int64_t* F = ids + PED_FATHER * stride; const int64_t* FF = ids + PED_FF * stride; const int64_t* FM = ids + PED_FM * stride;
    const int64_t* MF = ids + PED_MF * stride; const int64_t* MM = ids + PED_MM * stride;
    const bool sib = F[a] == F[b];
    const bool cousin = FF[a] == FF[b] || FF[a] == MF[b] || MF[a] == FF[b] || MF[a] == MF[b] ||
                        FM[a] == FM[b] || FM[a] == MM[b] || MM[a] == FM[b] || MM[a] == MM[b];
    const u32 v = (sib || cousin) ? 1u : 0u;
    if (v) atomicAdd(stat + AMS_NINB, 1u);
    inb[i] = v;
}
