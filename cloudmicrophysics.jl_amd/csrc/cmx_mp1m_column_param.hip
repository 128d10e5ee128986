// cmx_mp1m_column_param.hip — the derivatives of the 1-moment column step with sedimentation (cmx_mp1m_column.hip, Instantaneous mode) with respect to the
// PARAMETERS, the fall-speed parameters and the two precipitation fluxes included, for gfx950: C-ABI entry points cmx_mp1m_column_param_jvp_* / _param_vjp_*
// (include/cmx.h §(28)).  What loss(precip_rai + precip_sno).backward() needs to reach theta (cmx/autograd.py).  The scheme and the bodies of one point are
// cmx_mp1m_column_param.hpp's, shared with the host test build; the kernels are the halo shell (J_θ δθ: 4·(1 + KP) halo values per point) and the chunk
// shell (the gradient, finished by launch_param_vjp_finish) of cmx_column_products.hpp, and here are their policy struct and the entries.
//
// A call is a sequence of launches of kCol1mParamK or one direction each (for_each_column_param_launch), for the gradient followed by one finish launch.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_column_products.hpp"
#include "cmx_mp1m_column_param.hpp"

namespace cmx {

// The parameter derivatives of the scheme S_ in the shells: KP directions per evaluation, in the tangent slots of the constants
template <typename S_, typename FT_, int KP> struct Mp1mColParamBody {
    using S = S_;
    using FT = FT_;
    using Consts = Col1mParamConsts<FT, KP>;
    using Args = Col1mParamJvpArgs<FT, KP>;
    using GradArgs = Col1mParamVjpArgs<FT>;
    using Point = Col1mParamPoint<FT, KP>;
    static constexpr int NT = KP;
    static constexpr bool TANGENTS = false;
    static __device__ __forceinline__ FT Fd(const Point &p, int k, int s) { return p.Fd[k][s]; }
    static __device__ __forceinline__ void eval(const Consts &c, const FT (&x)[S::NWRT + 1], const FT (&)[S::NWRT], FT inv_dz, Point &p) {
        column1m_param_eval<S, FT, KP>(c, x, inv_dz, p);
    }
    static __device__ __forceinline__ void store(const Args &a, const Point &p, const FT (&upv)[4], const FT (&upd)[KP][4], bool top, bool surface, int64_t i,
                                                 int64_t col) {
        column1m_param_jvp_store<S, FT, KP>(a, p, upv, upd, top, surface, i, col);
    }
    static __device__ __forceinline__ void grad_point(const Consts &c, const GradArgs &a, const FT (&x)[S::NWRT + 1], int64_t i, int64_t col, int32_t lev,
                                                      double (&acc)[KP]) {
        column1m_param_vjp_point<S, FT, KP>(c, a, x, i, col, lev, acc);
    }
};

// ---- host side -----------------------------------------------------------------------------------------------------
// The statuses both entries share, in the order of the §(27) entries and then of §(22): the parameters, then `status` — the ladder of column_entry_status
// with the operation's columns — then with_mp1m_column_param: finite directions, b and b_ρ of the Chen-2022 rain table.  run(S, x, n): x are the columns, NULLs
// when there is no point.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI, typename RUN>
static int32_t param_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int32_t status, int64_t n_col,
                           int32_t n_lev, const FT *const *in, int32_t ndir, const MP *d_mp, const TH *d_tps, const ST *d_stokes, const CH *d_chen_rain,
                           const CI *d_chen_ice, RUN &&run) {
    if (!mp || !tps || !stokes || !chen_rain || !chen_ice) return CMX_ERR_BAD_ARG;
    if (status != kColumnEntryRun) return status;
    const FT *x[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int j = 0; n_col > 0 && j < 7; ++j) x[j] = in[j];
    return with_mp1m_column_param<FT>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, ndir, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice,
                                      [&](auto S) -> int32_t { return run(S, x, n_col * (int64_t)n_lev); });
}

template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t param_jvp_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev,
                               const FT *inv_dz, const FT *const *in, int32_t ndir, const MP *d_mp, const TH *d_tps, const ST *d_stokes, const CH *d_chen_rain,
                               const CI *d_chen_ice, FT *const *jvp, FT *const *jvp_precip_rai, FT *const *jvp_precip_sno, FT *const *tendencies, FT *precip_rai,
                               FT *precip_sno, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return param_entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags,
                           mp1m_column_param_jvp_status(flags, n_col, n_lev, inv_dz, in, ndir, d_mp, jvp, jvp_precip_rai, jvp_precip_sno, tendencies, precip_rai,
                                                        precip_sno),
                           n_col, n_lev, in, ndir, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice, [&](auto S, const FT *const (&x)[7], int64_t n) -> int32_t {
                               using SC = decltype(S);
                               for_each_column_param_launch<kCol1mParamK<FT, SC::general>>(ndir, [&](auto K, int d0) {
                                   constexpr int KP = decltype(K)::value;
                                   Col1mParamJvpArgs<FT, KP> a;
                                   if (!make_col1m_param_jvp_args(a, x, inv_dz, n, n_lev, d0, ndir, jvp, jvp_precip_rai, jvp_precip_sno, tendencies, precip_rai,
                                                                  precip_sno))
                                       return;
                                   Col1mParamConsts<FT, KP> c;
                                   make_col1m_param_consts<FT, KP>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice,
                                                                   d0, ndir, c);
                                   launch_column_halo<Mp1mColParamBody<SC, FT, KP>>(c, a, s);
                               });
                               return launched();
                           });
}

template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t param_vjp_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev,
                               const FT *inv_dz, const FT *const *in, const FT *const *cotangents, const FT *cot_precip_rai, const FT *cot_precip_sno, int32_t ndir,
                               const MP *d_mp, const TH *d_tps, const ST *d_stokes, const CH *d_chen_rain, const CI *d_chen_ice, double *grad, double *workspace,
                               FT *const *tendencies, FT *precip_rai, FT *precip_sno, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return param_entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags,
                           mp1m_column_param_vjp_status(flags, n_col, n_lev, inv_dz, in, cotangents, cot_precip_rai, cot_precip_sno, ndir, d_mp, grad, workspace,
                                                        tendencies, precip_rai, precip_sno),
                           n_col, n_lev, in, ndir, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice, [&](auto S, const FT *const (&x)[7], int64_t n) -> int32_t {
                               if (n == 0) {      // no point: the sums are zeros
                                   CMX_HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * (size_t)ndir, s));
                                   return (int32_t)CMX_OK;
                               }
                               using SC = decltype(S);
                               for_each_column_param_launch<kCol1mParamK<FT, SC::general>>(ndir, [&](auto K, int d0) {
                                   constexpr int KP = decltype(K)::value;
                                   Col1mParamConsts<FT, KP> c;
                                   make_col1m_param_consts<FT, KP>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice,
                                                                   d0, ndir, c);
                                   Col1mParamVjpArgs<FT> a;
                                   make_col1m_param_vjp_args(a, x, inv_dz, n, n_lev, cotangents, cot_precip_rai, cot_precip_sno, d0 == 0, tendencies, precip_rai,
                                                             precip_sno);
                                   launch_column_param_vjp<Mp1mColParamBody<SC, FT, KP>>(c, a, d0, ndir, workspace, s);
                               });
                               launch_param_vjp_finish(ndir, workspace, grad, s);
                               return launched();
                           });
}

}  // namespace cmx

#define CMX_COLUMN_PARAM_1M(SFX, FT)                                                                                                                                   \
    int32_t cmx_mp1m_column_param_jvp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *stokes,                      \
                                            const cmx_chen2022_rain_vel_##SFX *chen_rain, const cmx_chen2022_ice_vel_##SFX *chen_ice, uint32_t flags, int64_t n_col,   \
                                            int32_t n_lev, const FT *inv_dz, const FT *const *in, int32_t ndir, const cmx_microphysics_1m_##SFX *d_mp,                 \
                                            const cmx_thermo_##SFX *d_tps, const cmx_stokes_vel_##SFX *d_stokes, const cmx_chen2022_rain_vel_##SFX *d_chen_rain,       \
                                            const cmx_chen2022_ice_vel_##SFX *d_chen_ice, FT *const *jvp, FT *const *jvp_precip_rai, FT *const *jvp_precip_sno,        \
                                            FT *const tendencies[CMX_MP1M_JAC_NOUT], FT *precip_rai, FT *precip_sno, void *stream) {                                   \
        return cmx::param_jvp_entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, in, ndir, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice,   \
                                        jvp, jvp_precip_rai, jvp_precip_sno, tendencies, precip_rai, precip_sno, stream);                                              \
    }                                                                                                                                                                  \
    int32_t cmx_mp1m_column_param_vjp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *stokes,                      \
                                            const cmx_chen2022_rain_vel_##SFX *chen_rain, const cmx_chen2022_ice_vel_##SFX *chen_ice, uint32_t flags, int64_t n_col,   \
                                            int32_t n_lev, const FT *inv_dz, const FT *const *in, const FT *const cotangents[CMX_MP1M_JAC_NOUT],                       \
                                            const FT *cot_precip_rai, const FT *cot_precip_sno, int32_t ndir, const cmx_microphysics_1m_##SFX *d_mp,                   \
                                            const cmx_thermo_##SFX *d_tps, const cmx_stokes_vel_##SFX *d_stokes, const cmx_chen2022_rain_vel_##SFX *d_chen_rain,       \
                                            const cmx_chen2022_ice_vel_##SFX *d_chen_ice, double *grad, double *workspace, FT *const tendencies[CMX_MP1M_JAC_NOUT],    \
                                            FT *precip_rai, FT *precip_sno, void *stream) {                                                                            \
        return cmx::param_vjp_entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, in, cotangents, cot_precip_rai, cot_precip_sno, ndir, d_mp, \
                                        d_tps, d_stokes, d_chen_rain, d_chen_ice, grad, workspace, tendencies, precip_rai, precip_sno, stream);                        \
    }

extern "C" {
CMX_COLUMN_PARAM_1M(f32, float)
CMX_COLUMN_PARAM_1M(f64, double)
}
