// gev_select.h -- Simulation::ras_compute_mating_value_selection_value (reference src/Simulation.cpp:3300-3342) with
// Simulation::ras_selection_func (:3386-3428) on the device, one thread per individual.  Included by gev_library.hip after
// gev_kernels.h.  Built with -ffp-contract=off like the rest of the library: every multiply and add rounds on its own, as the
// reference's scalar FP64 code does.  exp / erf / sqrt / pow are the device's FP64 libm (within an ulp or so of glibc's).
#pragma once

#define GEV_SEL_MAX_PHEN 64

// per-call constants, passed by value (no upload, no host wait)
struct SelArgs {
    double omega[GEV_SEL_MAX_PHEN], lambda[GEV_SEL_MAX_PHEN], shift[GEV_SEL_MAX_PHEN];
    double par1, par2;
    int nphen, func, gen_num, reserved;
};

// ras_selection_func for one standardised value z (generation >= 1); CommFunc::NormalCDF / NormalPDF (src/CommFunc.cpp:257-270)
__device__ __forceinline__ double sel_func(const SelArgs& a, double z)
{
    if (a.gen_num == 0) return 1;                                   // :3388-3389
    switch (a.func) {
    case GEV_SEL_DEFAULT: { const double y = exp(0.0 + 1.0 * z); return y / (1 + y); }           // "" = logit 0 1 (:3393-3399)
    case GEV_SEL_LOGIT:   { const double y = exp(a.par1 + a.par2 * z); return y / (1 + y); }     // NaN where exp overflows (:3400-3406)
    case GEV_SEL_PROBIT:  return .5 * (1 + erf((z - a.par1) / (sqrt(2.0) * a.par2)));
    case GEV_SEL_STAB:    { const double pi = 3.1415926;                                          // the reference's constant (CommFunc.cpp:4)
                            return 1 / (sqrt(2.0 * pi) * a.par2) * exp(-0.5 * pow((z - a.par1) / a.par2, 2)); }
    case GEV_SEL_THR:     return z <= a.par2 ? a.par1 : 1.0;                                       // p1 below the threshold, 1 above (:3420-3426)
    default:              return 1;                                                                // GEV_SEL_NONE
    }
}
// sv standardised to generation 0 (:3333-3336): sv0 = {mean, var}
__device__ __forceinline__ double sel_standardise(double sv, const double* sv0)
{
    const double mean = sv0[0], var = sv0[1];
    double z = sv - mean;
    if (var > 0) z = (sv - mean) / sqrt(var);
    return z;
}

// mv = sum omega[p] * phen[p], sv = sum lambda[p] * phen[p] in phenotype order (:3310-3318); phen[p] includes the --gamma constant
// of the population (:3291), added first as the reference adds it to Human::phen.  finish != 0 (generation > 0, or generation-0
// statistics already known): standardise and apply the function here; else sv is left raw for the generation-0 reduction (k_ph_var_*).
__global__ void __launch_bounds__(256) k_sel_values(const double* __restrict__ phen, size_t n, SelArgs a, const double* __restrict__ sv0, int finish,
                                                    double* __restrict__ mv_out, double* __restrict__ sv_out, double* __restrict__ svf_out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double mv = 0, sv = 0;
    for (int p = 0; p < a.nphen; p++) {
        const double x = phen[i * (size_t)a.nphen + p] + a.shift[p];
        mv += a.omega[p] * x;
        sv += a.lambda[p] * x;
    }
    mv_out[i] = mv;
    if (finish) { const double z = sel_standardise(sv, sv0); sv_out[i] = z; svf_out[i] = sel_func(a, z); }
    else sv_out[i] = sv;
}
__global__ void __launch_bounds__(256) k_sel_finish(size_t n, SelArgs a, const double* __restrict__ sv0, double* __restrict__ sv, double* __restrict__ svf_out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double z = sel_standardise(sv[i], sv0);
    sv[i] = z; svf_out[i] = sel_func(a, z);
}
__global__ void k_sel_set_gen0(double* __restrict__ out, double mean, double var)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { out[0] = mean; out[1] = var; }
}
// rows of `width` doubles of src selected by map (positions) into dst: the values follow the migrants (gev_migrate)
__global__ void k_gather_f64(double* __restrict__ dst, const double* __restrict__ src, const u32* __restrict__ map, size_t n, u32 width)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * width) return;
    const size_t i = t / width, k = t - i * width;
    dst[t] = src[(size_t)map[i] * width + k];
}
