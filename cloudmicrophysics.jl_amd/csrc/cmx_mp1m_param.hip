// cmx_mp1m_param.hip — the derivatives of the 1-moment tendencies with respect to the PARAMETERS, for gfx950: C-ABI entry points
// cmx_mp1m_param_jvp_* / _param_vjp_* (include/cmx.h §(23)), the twin of cmx_sb2006_param.hip.  The point function is mp1m_point, the scheme Mp1mJac and the kernels the shared
// driver's (param_jvp_kernel / param_vjp_kernel, cmx_jacobian.hpp): the state enters as constants, the constants struct holds duals whose tangents the host
// forms per direction in exact forward mode (make_mp1m_param_consts, cmx_mp1m_jacobian.hpp) and passes as the first kernel argument.  A call is
// a sequence of launches of kParamK<FT> or one direction each (for_each_param_launch), for the gradient followed by one finish launch.  A translation unit of its own: no other kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_mp1m_jacobian.hpp"

namespace cmx {

#ifndef CMX_PARAM1M_BS
#define CMX_PARAM1M_BS 256
#endif
constexpr int kParam1mBS = CMX_PARAM1M_BS, kNOut = CMX_MP1M_JAC_NOUT, kNWrt = CMX_MP1M_JAC_NWRT;

template <typename FT, typename WR, typename TH>
static int32_t param_jvp_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], int32_t ndir, const WR *d_wr, const TH *d_tps,
                               FT *const *jvp, FT *const *tendencies, void *stream) {
    if (!wr || !tps) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT_LIMIT(n);
    if (const int32_t st = check_flags_1m(flags)) return st;
    if (n == 0) return CMX_OK;
    for (const FT *p : in)
        if (!p) return CMX_ERR_BAD_ARG;
    if (ndir < 1 || ndir > CMX_PARAM_MAX_DIRS || !d_wr) return CMX_ERR_BAD_ARG;
    bool any = false;
    for (int q = 0; q < ndir * kNOut && jvp; ++q) any |= jvp[q] != nullptr;
    for (int q = 0; q < kNOut && tendencies; ++q) any |= tendencies[q] != nullptr;
    if (!any) return CMX_ERR_BAD_ARG;
    return with_mp1m_param<FT>(*wr, *tps, flags, ndir, d_wr, d_tps, [&](auto S) {
        using SJ = decltype(S);
        for_each_param_launch<FT>(ndir, [&](auto K, int d0) {
            constexpr int KP = decltype(K)::value;
            using CD = Mp1mConsts<Dual<FT, KP>>;
            const CD cd = make_mp1m_param_consts<FT, KP>(*wr, *tps, flags, d_wr, d_tps, d0, ndir);
            ParamJvpArgs<FT, KP, kNOut, kNWrt> a{};
            bool wanted = false;
            for (int j = 0; j < kNWrt + 1; ++j) a.in[j] = in[j];
            for (int q = 0; q < kNOut; ++q) wanted |= (a.tend[q] = d0 == 0 && tendencies ? tendencies[q] : nullptr) != nullptr;      // the primal: the first launch's
            for (int k = 0; k < KP && d0 + k < ndir && jvp; ++k)
                for (int q = 0; q < kNOut; ++q) wanted |= (a.jvp[k][q] = jvp[(d0 + k) * kNOut + q]) != nullptr;
            if (wanted) launch<kParam1mBS>(param_jvp_kernel<SJ, FT, KP, kParam1mBS, CD>, n, reinterpret_cast<hipStream_t>(stream), cd, a, n);
        });
        return launched();
    });
}

template <typename FT, typename WR, typename TH>
static int32_t param_vjp_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], const FT *const *cotangents, int32_t ndir,
                               const WR *d_wr, const TH *d_tps, double *grad, double *workspace, FT *const *tendencies, void *stream) {
    static_assert(kParam1mBS * 4 == CMX_PARAM_VJP_PARTIALS, "the finish launch gives each lane four partials");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!wr || !tps) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT_LIMIT(n);
    if (const int32_t st = check_flags_1m(flags)) return st;
    // n = 0 writes grad, so it is checked like any other call except for the columns, which it does not read
    for (const FT *p : in)
        if (n > 0 && !p) return CMX_ERR_BAD_ARG;
    if (ndir < 1 || ndir > CMX_PARAM_MAX_DIRS || !d_wr || !cotangents) return CMX_ERR_BAD_ARG;
    if (!grad || !workspace) return CMX_ERR_BAD_ARG;
    return with_mp1m_param<FT>(*wr, *tps, flags, ndir, d_wr, d_tps, [&](auto S) -> int32_t {
        if (n == 0) {      // no point: the sums are zeros
            CMX_HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * (size_t)ndir, s));
            return (int32_t)CMX_OK;
        }
        using SJ = decltype(S);
        const int64_t chunk = param_vjp_chunk(n, kParam1mBS);
        for_each_param_launch<FT>(ndir, [&](auto K, int d0) {
            constexpr int KP = decltype(K)::value;
            using CD = Mp1mConsts<Dual<FT, KP>>;
            const CD cd = make_mp1m_param_consts<FT, KP>(*wr, *tps, flags, d_wr, d_tps, d0, ndir);
            ParamVjpArgs<FT, kNOut, kNWrt> a{};
            for (int j = 0; j < kNWrt + 1; ++j) a.in[j] = in[j];
            for (int q = 0; q < kNOut; ++q) {
                a.cot[q] = cotangents[q];
                a.ncot += cotangents[q] != nullptr;
                a.tend[q] = d0 == 0 && tendencies ? tendencies[q] : nullptr;
            }
            const int32_t nlive = ndir - d0 < KP ? ndir - d0 : KP;
            launch_grid(param_vjp_kernel<SJ, FT, KP, kParam1mBS, CD>, dim3(CMX_PARAM_VJP_PARTIALS), dim3(kParam1mBS), 0, s, cd, a, n, chunk, nlive,
                        workspace + (int64_t)d0 * CMX_PARAM_VJP_PARTIALS);
        });
        launch_grid(param_vjp_finish_kernel<kParam1mBS>, dim3((unsigned)ndir), dim3(kParam1mBS), 0, s, static_cast<const double *>(workspace), grad);
        return launched();
    });
}

}  // namespace cmx

extern "C" {
#define CMX_MP1M_PARAM_ENTRIES(SFX, FT)                                                                                                                          \
    int32_t cmx_mp1m_param_jvp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, uint32_t flags, int64_t n_points, const FT *rho,          \
                                     const FT *T, const FT *q_tot, const FT *q_lcl, const FT *q_icl, const FT *q_rai, const FT *q_sno, int32_t ndir,              \
                                     const cmx_microphysics_1m_##SFX *d_mp, const cmx_thermo_##SFX *d_tps, FT *const *jvp,                                         \
                                     FT *const tendencies[CMX_MP1M_JAC_NOUT], void *stream) {                                                                     \
        return cmx::param_jvp_entry<FT>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, ndir, d_mp, d_tps, jvp, tendencies, stream);      \
    }                                                                                                                                                            \
    int32_t cmx_mp1m_param_vjp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, uint32_t flags, int64_t n_points, const FT *rho,          \
                                     const FT *T, const FT *q_tot, const FT *q_lcl, const FT *q_icl, const FT *q_rai, const FT *q_sno,                            \
                                     const FT *const cotangents[CMX_MP1M_JAC_NOUT], int32_t ndir, const cmx_microphysics_1m_##SFX *d_mp,                           \
                                     const cmx_thermo_##SFX *d_tps, double *grad, double *workspace, FT *const tendencies[CMX_MP1M_JAC_NOUT], void *stream) {     \
        return cmx::param_vjp_entry<FT>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, cotangents, ndir, d_mp, d_tps, grad, workspace,   \
                                        tendencies, stream);                                                                                                     \
    }
CMX_MP1M_PARAM_ENTRIES(f32, float)
CMX_MP1M_PARAM_ENTRIES(f64, double)
#undef CMX_MP1M_PARAM_ENTRIES
}
