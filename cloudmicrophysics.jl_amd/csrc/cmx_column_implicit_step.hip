// cmx_column_implicit_step.hip — the column steps with the sub-stepped implicit average as tendency operator AND backward-Euler upwind sedimentation, stable
// and positive at any Courant number: C-ABI entry points cmx_sb2006_column_implicit_step_* and cmx_mp1m_column_implicit_step_* (include/cmx.h §(21)).  Per
// point the average a_j of §(19) and the fluxes F_j, g of §(20), bit for bit as in cmx_column_implicit_average.hip; then per species, with the fall speed w the
// flux function multiplied into F,
//     τ = Δt·w   c = τ·inv_dz[k]   β = τ·ρ⁺   r = 1/(1 + c)   A = c·r   B = fma(β, a, F)·r
//     G_k = top ? B_k : fma(A_k, G_{k+1}, B_k)                     from the column top downward
//     out_k = fma(top ? 0 : G_{k+1}, g, fma(−F_k, g, a_k))·r_k     surface output: G_0
// r is a TRUE division (exactly 1 at c = 0); the fall speeds are those of the initial state.
//
// Kernel shape: the recurrence runs down a column, so a workgroup OWNS a contiguous range of whole columns (cols_per_wg of them, a host-side tuning number
// that no result depends on) and no workgroup ever waits for another.  It walks its range in chunks of BS flat points from the highest index to the lowest.
// Per chunk
//   1. parallel — one point per lane, as in cmx_column_implicit_average.hip: the substeps (implicit_average_substeps, cmx_jacobian.hpp: the loop
//      of the average entry itself), then the (F, w) flux function of the scheme (sed_fluxes_w_of_point, mp1m_sed_fluxes_w: the operations of the
//      flux-only functions on the same operands).  The lane forms A and B, stores them to LDS at once and keeps fma(−F, g, a), g and r: the Float64 instantiations have no register to
//      spare.  Barrier.
//   2. serial — one lane per (column segment inside the chunk, species) runs G = fma(A, G_up, B) down its segment: one dependent fma per level, the A and B
//      reads do not depend on the chain.  A segment that starts below a column top takes G_up from the carry of the chunk before (LDS, two slots used in
//      turn so that the lane that writes the next carry never races the lane that reads this one); a column longer than a chunk is simply several chunks.
//      Being sequential by definition is what makes the result independent of tiling.  Barrier.
//   3. parallel — every lane reads G_{k+1} and stores `out`; the lane at level 0 stores G_0.
// The flux options are wave-uniform run-time branches, the tendency options template arguments through the average entries' own dispatch, as in the sibling:
// 8 + 4 kernels.  The outputs must not alias the inputs (the entries keep the rule of §(20)).
// The flux side of each scheme, the kernel-argument struct and the entry layer — so the statuses of the §(20) entries, in their order — are
// cmx_column_implicit.hpp's, shared with the sibling; here are the kernel, its launch and the extern "C" functions.  The kernel's body is text
// (cmx_column_implicit_step_body.inc) and its IO struct a header (cmx_column_implicit_step_kernel.hpp): the ensemble form of include/cmx.h §(29),
// cmx_column_implicit_step_ensemble.hip, includes both.
#include "cmx_column_implicit_step_kernel.hpp"

namespace cmx {

// Float32: compiled for four waves per SIMD, where cmx_column_implicit_average.hip runs (without the request 130–134 registers, three waves: 1-moment 0.82 → 0.76 ms,
// SB2006 0.69 → 0.66 ms per 1e7 points at nsub = 1; no vector register spills, no scratch instruction).  Float64 sits at one wave per SIMD either way.
template <typename S, typename FX, typename FT, int K, int BS>
__global__ __launch_bounds__(BS, sizeof(FT) == 4 ? 4 : 1) void implicit_sedimentation_step_kernel(const ImplicitColumnArgs<S, FX, FT, K, ImplicitStepIO<FT>> k0) {
#define CMX_ISTEP_TEND_CONSTS k0.ka.c
#define CMX_ISTEP_FLUX_CONSTS k0.ka
#define CMX_ISTEP_AVG_ARGS k0.a
#define CMX_ISTEP_IO0 k0.io
#define CMX_ISTEP_ARGS_AFTER(dep) consts_after(front_consts<FT, true>(k0), dep)
#define CMX_ISTEP_IN_INDEX(i) (i)
#define CMX_ISTEP_COL_ORIGIN(io) 0
#define CMX_ISTEP_NT_IN true
#include "cmx_column_implicit_step_body.inc"
#undef CMX_ISTEP_TEND_CONSTS
#undef CMX_ISTEP_FLUX_CONSTS
#undef CMX_ISTEP_AVG_ARGS
#undef CMX_ISTEP_IO0
#undef CMX_ISTEP_ARGS_AFTER
#undef CMX_ISTEP_IN_INDEX
#undef CMX_ISTEP_COL_ORIGIN
#undef CMX_ISTEP_NT_IN
}

// ---- host side -----------------------------------------------------------------------------------------------------
// (n_col ≤ kMaxPoints / n_lev and at least 16 points per workgroup — n_lev ≥ 16, or ≥ 512 columns of fewer levels — keep the grid inside HIP's 2^31 − 1)
template <typename FT> static dim3 step_grid(const ImplicitStepIO<FT> &io) { return dim3((unsigned)tile_grid(io.n_col, io.cols_per_wg)); }

// the callable of the entry layer (cmx_column_implicit.hpp): the IO struct and the launch
template <typename FT> static auto step_launch(const FT *inv_dz, FT *precip0, FT *precip1, int64_t n_col, int32_t n_lev, double dt, void *stream) {
    return [=](auto scheme, auto fx, const auto &ka, const auto &a, int32_t opt0, int32_t opt1) -> int32_t {
        constexpr int K = kImplicitAvgK<FT>;
        const ImplicitColumnArgs<decltype(scheme), decltype(fx), FT, K, ImplicitStepIO<FT>> k{ka, a, make_io<FT>(inv_dz, precip0, precip1, n_col, n_lev, opt0, opt1, dt)};
        launch_grid(implicit_sedimentation_step_kernel<decltype(scheme), decltype(fx), FT, K, kImplStepBS>, step_grid(k.io), dim3(kImplStepBS), 0,
                    reinterpret_cast<hipStream_t>(stream), k);
        return launched();
    };
}

}  // namespace cmx

extern "C" {
int32_t cmx_sb2006_column_implicit_step_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                            const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags, int64_t n_col,
                                            int32_t n_lev, const float *inv_dz, const float *rho, const float *T, const float *q_tot, const float *q_lcl,
                                            const float *n_lcl, const float *q_rai, const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt,
                                            float *dn_rai_dt, float *precip_flux, void *stream) {
    return cmx::sb2006_implicit_column_entry<float>(warm_rain, tps, vel, cloud_vel, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz,
                                                    {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, {dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt},
                                                    cmx::step_launch<float>(inv_dz, precip_flux, nullptr, n_col, n_lev, dt, stream));
}
int32_t cmx_sb2006_column_implicit_step_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                            const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags, int64_t n_col,
                                            int32_t n_lev, const double *inv_dz, const double *rho, const double *T, const double *q_tot, const double *q_lcl,
                                            const double *n_lcl, const double *q_rai, const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt,
                                            double *dq_rai_dt, double *dn_rai_dt, double *precip_flux, void *stream) {
    return cmx::sb2006_implicit_column_entry<double>(warm_rain, tps, vel, cloud_vel, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz,
                                                     {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, {dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt},
                                                     cmx::step_launch<double>(inv_dz, precip_flux, nullptr, n_col, n_lev, dt, stream));
}
int32_t cmx_mp1m_column_implicit_step_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                          const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags, double dt,
                                          int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *const *in,
                                          float *const *out, float *precip_rai, float *precip_sno, void *stream) {
    return cmx::mp1m_implicit_column_entry<float>(mp, tps, stokes, chen_rain, chen_ice, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out,
                                                  cmx::step_launch<float>(inv_dz, precip_rai, precip_sno, n_col, n_lev, dt, stream));
}
int32_t cmx_mp1m_column_implicit_step_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                          const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags, double dt,
                                          int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *const *in,
                                          double *const *out, double *precip_rai, double *precip_sno, void *stream) {
    return cmx::mp1m_implicit_column_entry<double>(mp, tps, stokes, chen_rain, chen_ice, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out,
                                                   cmx::step_launch<double>(inv_dz, precip_rai, precip_sno, n_col, n_lev, dt, stream));
}
}
