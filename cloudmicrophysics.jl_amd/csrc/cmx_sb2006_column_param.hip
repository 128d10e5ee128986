// cmx_sb2006_column_param.hip — the derivatives of the SB2006 column step with sedimentation (cmx_sb2006_column.hip) with respect to the PARAMETERS, the
// fall-speed parameters and the precipitation flux included, for gfx950: C-ABI entry points cmx_sb2006_column_param_jvp_* / _param_vjp_* (include/cmx.h
// §(26)).  What loss(precip_flux).backward() needs to reach theta (cmx/autograd.py).  The scheme and the bodies of one point are
// cmx_sb2006_column_param.hpp's, shared with the host test build; the kernels are the halo shell (J_θ δθ: 4·(1 + KP) halo values per point) and the chunk
// shell (the gradient, finished by launch_param_vjp_finish) of cmx_column_products.hpp, and here are their policy struct and the entries.
// (The alternative to the halo, a flux-only re-evaluation of the point above on duals, was not built: it repeats the rain PSD and both fall speeds with KP
// tangents for every point, where the halo costs one extra lane in 256 and at most 24 KiB of LDS per workgroup — below what limits the waves of kernels with
// these register counts.)
//
// A call is a sequence of launches of kColParamK or one direction each (for_each_column_param_launch), for the gradient followed by one finish launch.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_column_products.hpp"
#include "cmx_sb2006_column_param.hpp"

namespace cmx {

// The parameter derivatives of the scheme S_ in the shells: KP directions per evaluation, in the tangent slots of the constants
template <typename S_, typename FT_, int KP> struct SbColParam {
    using S = S_;
    using FT = FT_;
    using Consts = SbColConsts<Dual<FT, KP>>;
    using Args = ColParamJvpArgs<FT, KP>;
    using GradArgs = ColParamVjpArgs<FT>;
    using Point = ColParamPoint<FT, KP>;
    static constexpr int NT = KP;
    static constexpr bool TANGENTS = false;
    static __device__ __forceinline__ FT Fd(const Point &p, int k, int s) { return p.Fd[k][s]; }
    static __device__ __forceinline__ void eval(const Consts &k, const FT (&x)[S::NWRT + 1], const FT (&)[S::NWRT], FT inv_dz, Point &p) {
        column_param_eval<S, FT, KP>(k.c, k.cv, x, inv_dz, p);
    }
    static __device__ __forceinline__ void store(const Args &a, const Point &p, const FT (&upv)[4], const FT (&upd)[KP][4], bool top, bool surface, int64_t i,
                                                 int64_t col) {
        column_param_jvp_store<S, FT, KP>(a, p, upv, upd, top, surface, i, col);
    }
    static __device__ __forceinline__ void grad_point(const Consts &k, const GradArgs &a, const FT (&x)[S::NWRT + 1], int64_t i, int64_t col, int32_t lev,
                                                      double (&acc)[KP]) {
        column_param_vjp_point<S, FT, KP>(k.c, k.cv, a, x, i, col, lev, acc);
    }
};

// ---- host side -----------------------------------------------------------------------------------------------------
// The statuses both entries share, in the order of the primal column entry and then of §(22): the parameters, then `status` — the ladder of
// column_entry_status with the operation's columns — then with_sb2006_column_param: finite directions, the Chen-2022 table, the limiters, the fall-speed
// parameters.
template <typename FT, typename WR, typename TH, typename VL, typename ST, typename RUN>
static int32_t param_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int32_t status, int32_t ndir, const WR *d_wr,
                           const TH *d_tps, const VL *d_vel, const ST *d_cloud_vel, RUN &&run) {
    if (!wr || !tps || !vel) return CMX_ERR_BAD_ARG;
    if (status != kColumnEntryRun) return status;
    return with_sb2006_column_param<FT>(*wr, *tps, *vel, cloud_vel, flags, ndir, d_wr, d_tps, d_vel, d_cloud_vel, run);
}

template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t param_jvp_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
                               const FT *const (&in)[7], int32_t ndir, const WR *d_wr, const TH *d_tps, const VL *d_vel, const ST *d_cloud_vel, FT *const *jvp,
                               FT *const *jvp_precip, FT *const *tendencies, FT *precip, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return param_entry<FT>(wr, tps, vel, cloud_vel, flags,
                           sb2006_column_param_jvp_status(flags, n_col, n_lev, inv_dz, in, ndir, d_wr, jvp, jvp_precip, tendencies, precip), ndir, d_wr, d_tps,
                           d_vel, d_cloud_vel, [&](auto S) -> int32_t {
                               const int64_t n = n_col * (int64_t)n_lev;
                               using SC = decltype(S);
                               for_each_column_param_launch<kColParamK<FT, SC::vel>>(ndir, [&](auto K, int d0) {
                                   constexpr int KP = decltype(K)::value;
                                   SbColConsts<Dual<FT, KP>> k;
                                   make_column_param_consts<FT, KP>(*wr, *tps, *vel, cloud_vel, d_wr, d_tps, d_vel, d_cloud_vel, d0, ndir, k.c, k.cv);
                                   ColParamJvpArgs<FT, KP> a;
                                   if (!make_column_param_jvp_args(a, in, inv_dz, n, n_lev, d0, ndir, jvp, jvp_precip, tendencies, precip)) return;
                                   launch_column_halo<SbColParam<SC, FT, KP>>(k, a, s);
                               });
                               return launched();
                           });
}

template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t param_vjp_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
                               const FT *const (&in)[7], const FT *const *cotangents, const FT *cot_precip, int32_t ndir, const WR *d_wr, const TH *d_tps,
                               const VL *d_vel, const ST *d_cloud_vel, double *grad, double *workspace, FT *const *tendencies, FT *precip, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return param_entry<FT>(wr, tps, vel, cloud_vel, flags,
                           sb2006_column_param_vjp_status(flags, n_col, n_lev, inv_dz, in, cotangents, cot_precip, ndir, d_wr, grad, workspace, tendencies, precip),
                           ndir, d_wr, d_tps, d_vel, d_cloud_vel, [&](auto S) -> int32_t {
                               const int64_t n = n_col * (int64_t)n_lev;
                               if (n == 0) {      // no point: the sums are zeros
                                   CMX_HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * (size_t)ndir, s));
                                   return (int32_t)CMX_OK;
                               }
                               using SC = decltype(S);
                               // the Float64 gradient kernel of the general Chen-2022 instantiation (run-time Γ) needs 482–511 VGPRs at one direction per
                               // evaluation and spills 8: not shipped (cmx_sb2006_column_param.hpp has the table)
                               if constexpr (sizeof(FT) == 8 && SC::vel == VEL_CHEN_GEN) return (int32_t)CMX_ERR_UNSUPPORTED;
                               else {
                               for_each_column_param_launch<kColParamK<FT, SC::vel>>(ndir, [&](auto K, int d0) {
                                   constexpr int KP = decltype(K)::value;
                                   SbColConsts<Dual<FT, KP>> k;
                                   make_column_param_consts<FT, KP>(*wr, *tps, *vel, cloud_vel, d_wr, d_tps, d_vel, d_cloud_vel, d0, ndir, k.c, k.cv);
                                   ColParamVjpArgs<FT> a;
                                   make_column_param_vjp_args<SC>(a, in, inv_dz, n, n_lev, cotangents, cot_precip, d0 == 0, tendencies, precip);
                                   launch_column_param_vjp<SbColParam<SC, FT, KP>>(k, a, d0, ndir, workspace, s);
                               });
                               launch_param_vjp_finish(ndir, workspace, grad, s);
                               return launched();
                               }
                           });
}

}  // namespace cmx

#define CMX_COLUMN_PARAM(SFX, FT)                                                                                                                                      \
    int32_t cmx_sb2006_column_param_jvp_##SFX(const cmx_warm_rain_2m_##SFX *warm_rain, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                     \
                                              const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *rho,    \
                                              const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl, const FT *q_rai, const FT *n_rai, int32_t ndir,          \
                                              const cmx_warm_rain_2m_##SFX *d_warm_rain, const cmx_thermo_##SFX *d_tps, const cmx_rain_vel_##SFX *d_vel,               \
                                              const cmx_stokes_vel_##SFX *d_cloud_vel, FT *const *jvp, FT *const *jvp_precip,                                          \
                                              FT *const tendencies[CMX_SB2006_JAC_NOUT], FT *precip_flux, void *stream) {                                              \
        return cmx::param_jvp_entry<FT>(warm_rain, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, ndir, d_warm_rain,   \
                                        d_tps, d_vel, d_cloud_vel, jvp, jvp_precip, tendencies, precip_flux, stream);                                                  \
    }                                                                                                                                                                  \
    int32_t cmx_sb2006_column_param_vjp_##SFX(const cmx_warm_rain_2m_##SFX *warm_rain, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                     \
                                              const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *rho,    \
                                              const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl, const FT *q_rai, const FT *n_rai,                        \
                                              const FT *const cotangents[CMX_SB2006_JAC_NOUT], const FT *cot_precip, int32_t ndir,                                     \
                                              const cmx_warm_rain_2m_##SFX *d_warm_rain, const cmx_thermo_##SFX *d_tps, const cmx_rain_vel_##SFX *d_vel,               \
                                              const cmx_stokes_vel_##SFX *d_cloud_vel, double *grad, double *workspace, FT *const tendencies[CMX_SB2006_JAC_NOUT],     \
                                              FT *precip_flux, void *stream) {                                                                                         \
        return cmx::param_vjp_entry<FT>(warm_rain, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, cotangents,          \
                                        cot_precip, ndir, d_warm_rain, d_tps, d_vel, d_cloud_vel, grad, workspace, tendencies, precip_flux, stream);                   \
    }

extern "C" {
CMX_COLUMN_PARAM(f32, float)
CMX_COLUMN_PARAM(f64, double)
}
