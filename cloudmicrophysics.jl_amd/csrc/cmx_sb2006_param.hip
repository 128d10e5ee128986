// cmx_sb2006_param.hip — the derivatives of the SB2006 warm-rain tendencies with respect to the PARAMETERS, for gfx950: C-ABI entry points
// cmx_sb2006_warm_rain_param_jvp_* / _param_vjp_* (include/cmx.h §(22)).  The point function is sb2006_point, the scheme SbJac and the kernels the shared
// driver's (param_jvp_kernel / param_vjp_kernel, cmx_jacobian.hpp): the state enters as constants, the constants struct holds duals whose tangents the host
// forms per direction in exact forward mode (make_sb_param_consts, cmx_sb2006_jacobian.hpp) and passes as the first kernel argument.  A call is
// a sequence of launches of kParamK<FT> or one direction each (for_each_param_launch), for the gradient followed by one finish launch.  A translation unit of its own: no other kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_sb2006_jacobian.hpp"

namespace cmx {

#ifndef CMX_PARAM_BS
#define CMX_PARAM_BS 256
#endif
constexpr int kParamBS = CMX_PARAM_BS, kNOut = CMX_SB2006_JAC_NOUT, kNWrt = CMX_SB2006_JAC_NWRT;

template <typename FT, typename WR, typename TH>
static int32_t param_jvp_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], int32_t ndir, const WR *d_wr, const TH *d_tps,
                               FT *const *jvp, FT *const *tendencies, void *stream) {
    if (!wr || !tps) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT(n);
    for (const FT *p : in)
        if (!p) return CMX_ERR_BAD_ARG;
    if (ndir < 1 || ndir > CMX_PARAM_MAX_DIRS || !d_wr) return CMX_ERR_BAD_ARG;
    bool any = false;
    for (int q = 0; q < ndir * kNOut && jvp; ++q) any |= jvp[q] != nullptr;
    for (int q = 0; q < kNOut && tendencies; ++q) any |= tendencies[q] != nullptr;
    if (!any) return CMX_ERR_BAD_ARG;
    return with_sb2006_param<FT>(*wr, *tps, flags, ndir, d_wr, d_tps, [&](auto S) {
        using SJ = decltype(S);
        for_each_param_launch<FT>(ndir, [&](auto K, int d0) {
            constexpr int KP = decltype(K)::value;
            using CD = SbConsts<Dual<FT, KP>>;
            const CD cd = make_sb_param_consts<FT, KP>(*wr, *tps, d_wr, d_tps, d0, ndir);
            ParamJvpArgs<FT, KP, kNOut, kNWrt> a{};
            bool wanted = false;
            for (int j = 0; j < kNWrt + 1; ++j) a.in[j] = in[j];
            for (int q = 0; q < kNOut; ++q) wanted |= (a.tend[q] = d0 == 0 && tendencies ? tendencies[q] : nullptr) != nullptr;      // the primal: the first launch's
            for (int k = 0; k < KP && d0 + k < ndir && jvp; ++k)
                for (int q = 0; q < kNOut; ++q) wanted |= (a.jvp[k][q] = jvp[(d0 + k) * kNOut + q]) != nullptr;
            if (wanted) launch<kParamBS>(param_jvp_kernel<SJ, FT, KP, kParamBS, CD>, n, reinterpret_cast<hipStream_t>(stream), cd, a, n);
        });
        return launched();
    });
}

template <typename FT, typename WR, typename TH>
static int32_t param_vjp_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], const FT *const *cotangents, int32_t ndir,
                               const WR *d_wr, const TH *d_tps, double *grad, double *workspace, FT *const *tendencies, void *stream) {
    static_assert(kParamBS * 4 == CMX_PARAM_VJP_PARTIALS, "the finish launch gives each lane four partials");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!wr || !tps) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT_LIMIT(n);
    // n = 0 writes grad, so it is checked like any other call except for the columns, which it does not read
    for (const FT *p : in)
        if (n > 0 && !p) return CMX_ERR_BAD_ARG;
    if (ndir < 1 || ndir > CMX_PARAM_MAX_DIRS || !d_wr || !cotangents) return CMX_ERR_BAD_ARG;
    if (!grad || !workspace) return CMX_ERR_BAD_ARG;
    return with_sb2006_param<FT>(*wr, *tps, flags, ndir, d_wr, d_tps, [&](auto S) -> int32_t {
        if (n == 0) {      // no point: the sums are zeros
            CMX_HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * (size_t)ndir, s));
            return (int32_t)CMX_OK;
        }
        using SJ = decltype(S);
        const int64_t chunk = param_vjp_chunk(n, kParamBS);
        for_each_param_launch<FT>(ndir, [&](auto K, int d0) {
            constexpr int KP = decltype(K)::value;
            using CD = SbConsts<Dual<FT, KP>>;
            const CD cd = make_sb_param_consts<FT, KP>(*wr, *tps, d_wr, d_tps, d0, ndir);
            ParamVjpArgs<FT, kNOut, kNWrt> a{};
            for (int j = 0; j < kNWrt + 1; ++j) a.in[j] = in[j];
            for (int q = 0; q < kNOut; ++q) {
                a.cot[q] = cotangents[q];
                a.ncot += cotangents[q] != nullptr;
                a.tend[q] = d0 == 0 && tendencies ? tendencies[q] : nullptr;
            }
            const int32_t nlive = ndir - d0 < KP ? ndir - d0 : KP;
            launch_grid(param_vjp_kernel<SJ, FT, KP, kParamBS, CD>, dim3(CMX_PARAM_VJP_PARTIALS), dim3(kParamBS), 0, s, cd, a, n, chunk, nlive,
                        workspace + (int64_t)d0 * CMX_PARAM_VJP_PARTIALS);
        });
        launch_grid(param_vjp_finish_kernel<kParamBS>, dim3((unsigned)ndir), dim3(kParamBS), 0, s, static_cast<const double *>(workspace), grad);
        return launched();
    });
}

}  // namespace cmx

extern "C" {
int32_t cmx_sb2006_warm_rain_param_jvp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                           const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                           int32_t ndir, const cmx_warm_rain_2m_f32 *d_warm_rain, const cmx_thermo_f32 *d_tps, float *const *jvp,
                                           float *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::param_jvp_entry<float>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, ndir, d_warm_rain, d_tps, jvp, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_param_jvp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                           const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                           const double *n_rai, int32_t ndir, const cmx_warm_rain_2m_f64 *d_warm_rain, const cmx_thermo_f64 *d_tps,
                                           double *const *jvp, double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::param_jvp_entry<double>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, ndir, d_warm_rain, d_tps, jvp, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_param_vjp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                           const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                           const float *const cotangents[CMX_SB2006_JAC_NOUT], int32_t ndir, const cmx_warm_rain_2m_f32 *d_warm_rain,
                                           const cmx_thermo_f32 *d_tps, double *grad, double *workspace, float *const tendencies[CMX_SB2006_JAC_NOUT],
                                           void *stream) {
    return cmx::param_vjp_entry<float>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, cotangents, ndir, d_warm_rain, d_tps, grad,
                                       workspace, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_param_vjp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                           const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                           const double *n_rai, const double *const cotangents[CMX_SB2006_JAC_NOUT], int32_t ndir,
                                           const cmx_warm_rain_2m_f64 *d_warm_rain, const cmx_thermo_f64 *d_tps, double *grad, double *workspace,
                                           double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::param_vjp_entry<double>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, cotangents, ndir, d_warm_rain, d_tps, grad,
                                        workspace, tendencies, stream);
}
}

// Stage 2 of the parameter gradients for the other translation units that feed the reduction (cmx_sb2006_column_param.hip): the one instantiation of
// param_vjp_finish_kernel this file already launches.  (At the end of the file: the kernels are emitted in the order of their first use.)
namespace cmx {
void launch_param_vjp_finish(int32_t ndir, const double *workspace, double *grad, hipStream_t stream) {
    launch_grid(param_vjp_finish_kernel<kParamBS>, dim3((unsigned)ndir), dim3(kParamBS), 0, stream, workspace, grad);
}
}  // namespace cmx
