// cmx_sb2006_jacobian_products.hip — products with the Jacobian of the SB2006 warm-rain tendencies, for gfx950: J v (cmx_sb2006_warm_rain_jvp_*) and
// Jᵀḡ (cmx_sb2006_warm_rain_vjp_*), include/cmx.h §(16).  What a Jacobian-free Newton–Krylov matvec and a gradient (torch autograd, cmx/autograd.py)
// consume: 4 resp. 6 columns out instead of the 24 of cmx_sb2006_warm_rain_jacobian_* and a second pass that contracts them.
//
// The scheme is the Jacobian entry's, unchanged (SbJac, cmx_sb2006_jacobian.hpp: sb2006_point on the dual value type); the kernels and the point bodies
// are the shared driver's (jvp_kernel / vjp_kernel, cmx_jacobian_products.hpp).  One point per lane, the seven state columns read once, non-temporal;
// J v is ONE evaluation on Dual<FT, 1> seeded with the caller's tangent, Jᵀḡ is ⌈n_grad/K⌉ evaluations on Dual<FT, K> with unit seeds whose tangents are
// contracted with the cotangents in registers.  Stores are plain whole-column vector stores.  No LDS beyond the Float64 math tables, no inline assembly here.
//
// K of the VJP per float type (kVjpK below, -DCMX_VJP_K_F32=…, -DCMX_VJP_K_F64=…): the Jacobian entry's by default, from the register counts of a
// cross-compiled build (tools/kernel_resources.py; DESIGN.md §9 has the table).  A translation unit of its own: no existing kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_sb2006_jacobian.hpp"

namespace cmx {

#ifndef CMX_JAC_BS
#define CMX_JAC_BS 256
#endif
#ifndef CMX_VJP_K_F32
#define CMX_VJP_K_F32 CMX_JAC_K_F32
#endif
#ifndef CMX_VJP_K_F64
#define CMX_VJP_K_F64 CMX_JAC_K_F64
#endif
constexpr int kProdBS = CMX_JAC_BS;
template <typename FT> constexpr int kVjpK = sizeof(FT) == 4 ? CMX_VJP_K_F32 : CMX_VJP_K_F64;

// ---- host side -----------------------------------------------------------------------------------------------------
// The statuses of the Jacobian entry (cmx_sb2006_jacobian.hip), in its order; `table` = tangents / cotangents, which must not be NULL itself.
// make(a, in): fills the kernel's argument struct, false if the call has no output column at all.  run(c, a, L, I): the launch.
template <typename FT, typename ARGS, typename WR, typename TH, typename MAKE, typename RUN>
static int32_t product_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], const void *table, MAKE &&make, RUN &&run) {
    if (!wr || !tps) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT(n);
    for (const FT *p : in)
        if (!p) return CMX_ERR_BAD_ARG;
    ARGS a;
    if (!table || !make(a, in)) return CMX_ERR_BAD_ARG;      // no tangent / cotangent table, or no output column at all
    if (flags & ~(uint32_t)CMX_SB2006_LIMITED) return CMX_ERR_BAD_ARG;
    const bool limited = flags & CMX_SB2006_LIMITED;
    if (limited && !sb_limiters_ok(*wr)) return CMX_ERR_BAD_ARG;      // clamp_ordered needs ordered limiter pairs
    const SbConsts<FT> c = make_sb_consts<FT>(*wr, *tps, (const std::conditional_t<std::is_same_v<FT, float>, cmx_rain_vel_f32, cmx_rain_vel_f64> *)nullptr,
                                              (double)Math<FT>::eps_1m());
    const bool intpow = sb_integer_exponents(*wr);        // the instantiation the tendencies entry selects for the same parameter struct
    // One point per lane with 4- / 8-byte accesses: any alignment and any n go through one launch
    dispatch([&](auto L, auto I) { run(c, a, L, I); }, flag(limited), flag(intpow));
    return launched();
}

template <typename FT, typename WR, typename TH>
static int32_t jvp_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *rho, const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl,
                         const FT *q_rai, const FT *n_rai, const FT *const *tangents, FT *const *jvp, FT *const *tendencies, void *stream) {
    using A = JvpArgs<FT, CMX_SB2006_JAC_NOUT, CMX_SB2006_JAC_NWRT>;
    const FT *const in[7] = {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return product_entry<FT, A>(wr, tps, flags, n, in, tangents, [&](A &a, const FT *const (&x)[7]) { return make_jvp_args(a, x, tangents, jvp, tendencies); },
                                [&](const SbConsts<FT> &c, const A &a, auto L, auto I) {
                                    launch<kProdBS>(jvp_kernel<SbJac<decltype(L)::value, decltype(I)::value>, FT, kProdBS, SbConsts<FT>>, n, s, c, a, n);
                                });
}

template <typename FT, typename WR, typename TH>
static int32_t vjp_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *rho, const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl,
                         const FT *q_rai, const FT *n_rai, const FT *const *cotangents, FT *const *grad, FT *const *tendencies, void *stream) {
    constexpr int K = kVjpK<FT>;
    using A = VjpArgs<FT, K, CMX_SB2006_JAC_NOUT, CMX_SB2006_JAC_NWRT>;
    const FT *const in[7] = {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return product_entry<FT, A>(wr, tps, flags, n, in, cotangents, [&](A &a, const FT *const (&x)[7]) { return make_vjp_args(a, x, cotangents, grad, tendencies); },
                                [&](const SbConsts<FT> &c, const A &a, auto L, auto I) {
                                    launch<kProdBS>(vjp_kernel<SbJac<decltype(L)::value, decltype(I)::value>, FT, K, kProdBS, SbConsts<FT>>, n, s, c, a, n);
                                });
}

}  // namespace cmx

extern "C" {
int32_t cmx_sb2006_warm_rain_jvp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                     const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                     const float *const tangents[CMX_SB2006_JAC_NWRT], float *const jvp[CMX_SB2006_JAC_NOUT],
                                     float *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::jvp_entry<float>(warm_rain, tps, flags, n_points, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, tangents, jvp, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_jvp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                     const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai,
                                     const double *const tangents[CMX_SB2006_JAC_NWRT], double *const jvp[CMX_SB2006_JAC_NOUT],
                                     double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::jvp_entry<double>(warm_rain, tps, flags, n_points, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, tangents, jvp, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_vjp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                     const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                     const float *const cotangents[CMX_SB2006_JAC_NOUT], float *const grad[CMX_SB2006_JAC_NWRT],
                                     float *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::vjp_entry<float>(warm_rain, tps, flags, n_points, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, cotangents, grad, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_vjp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                     const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai,
                                     const double *const cotangents[CMX_SB2006_JAC_NOUT], double *const grad[CMX_SB2006_JAC_NWRT],
                                     double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::vjp_entry<double>(warm_rain, tps, flags, n_points, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, cotangents, grad, tendencies, stream);
}
}
