// cmx_mp1m_jacobian_products.hip — products with the Jacobian of the 1-moment tendencies, for gfx950: J v (cmx_mp1m_jvp_*) and Jᵀḡ (cmx_mp1m_vjp_*),
// include/cmx.h §(17).  What a Jacobian-free Newton–Krylov matvec and a gradient (torch autograd, cmx/autograd.py) consume: 4 resp. 6 columns out instead
// of the 24 of cmx_mp1m_jacobian_* and a second pass that contracts them.
//
// The scheme is the Jacobian entry's, unchanged (Mp1mJac<FLAGS>, cmx_mp1m_jacobian.hpp: mp1m_point + mp1m_aggregate on the dual value type); the kernels
// and the point bodies are the shared driver's (jvp_kernel / vjp_kernel, cmx_jacobian_products.hpp).  One point per lane, the seven state columns read
// once, non-temporal; J v is ONE evaluation on Dual<FT, 1> seeded with the caller's tangent, Jᵀḡ is ⌈n_grad/K⌉ evaluations on Dual<FT, K> with unit seeds
// whose tangents are contracted with the cotangents in registers.  Stores are plain whole-column vector stores.  No LDS beyond the Float64 math tables, no
// inline assembly here.
//
// FLAGS: the compile-time default-options / default-exponents instantiation or the run-time-flags one, chosen by flags_1m() as in cmx_mp1m_jacobian_*.
// K of the VJP per float type (kVjp1mK below, -DCMX_VJP1M_K_F32=…, -DCMX_VJP1M_K_F64=…): the Jacobian entry's by default, from the register counts of a
// cross-compiled build (tools/kernel_resources.py; DESIGN.md §9 has the table).  A translation unit of its own: no existing kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_mp1m_jacobian.hpp"

namespace cmx {

#ifndef CMX_JAC1M_BS
#define CMX_JAC1M_BS 256
#endif
#ifndef CMX_VJP1M_K_F32
#define CMX_VJP1M_K_F32 CMX_JAC1M_K_F32
#endif
#ifndef CMX_VJP1M_K_F64
#define CMX_VJP1M_K_F64 CMX_JAC1M_K_F64
#endif
constexpr int kProd1mBS = CMX_JAC1M_BS;
template <typename FT> constexpr int kVjp1mK = sizeof(FT) == 4 ? CMX_VJP1M_K_F32 : CMX_VJP1M_K_F64;

// ---- host side -----------------------------------------------------------------------------------------------------
// The statuses of the Jacobian entry (cmx_mp1m_jacobian.hip), in its order; `table` = tangents / cotangents, which must not be NULL itself.
// make(a, in): fills the kernel's argument struct, false if the call has no output column at all.  run(c, a, FL): the launch.
template <typename FT, typename ARGS, typename MP, typename TH, typename MAKE, typename RUN>
static int32_t product_1m_entry(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], const void *table, MAKE &&make, RUN &&run) {
    if (!mp || !tps) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT_LIMIT(n);
    if (const int32_t st = check_flags_1m(flags)) return st;
    if (n == 0) return CMX_OK;
    for (const FT *p : in)
        if (!p) return CMX_ERR_BAD_ARG;
    ARGS a;
    if (!table || !make(a, in)) return CMX_ERR_BAD_ARG;      // no tangent / cotangent table, or no output column at all
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(*mp, *tps, flags, (double)Math<FT>::eps_1m());
    // One point per lane with 4- / 8-byte accesses: any alignment and any n go through one launch
    dispatch([&](auto FL) { run(c, a, FL); }, flags_1m(flags, c));
    return launched();
}

template <typename FT, typename MP, typename TH>
static int32_t jvp_1m_entry(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *rho, const FT *T, const FT *q_tot, const FT *q_lcl, const FT *q_icl,
                            const FT *q_rai, const FT *q_sno, const FT *const *tangents, FT *const *jvp, FT *const *tendencies, void *stream) {
    using A = JvpArgs<FT, CMX_MP1M_JAC_NOUT, CMX_MP1M_JAC_NWRT>;
    const FT *const in[7] = {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return product_1m_entry<FT, A>(mp, tps, flags, n, in, tangents, [&](A &a, const FT *const (&x)[7]) { return make_jvp_args(a, x, tangents, jvp, tendencies); },
                                   [&](const Mp1mConsts<FT> &c, const A &a, auto FL) {
                                       launch<kProd1mBS>(jvp_kernel<Mp1mJac<decltype(FL)::value>, FT, kProd1mBS, Mp1mConsts<FT>>, n, s, c, a, n);
                                   });
}

template <typename FT, typename MP, typename TH>
static int32_t vjp_1m_entry(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *rho, const FT *T, const FT *q_tot, const FT *q_lcl, const FT *q_icl,
                            const FT *q_rai, const FT *q_sno, const FT *const *cotangents, FT *const *grad, FT *const *tendencies, void *stream) {
    constexpr int K = kVjp1mK<FT>;
    using A = VjpArgs<FT, K, CMX_MP1M_JAC_NOUT, CMX_MP1M_JAC_NWRT>;
    const FT *const in[7] = {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return product_1m_entry<FT, A>(mp, tps, flags, n, in, cotangents, [&](A &a, const FT *const (&x)[7]) { return make_vjp_args(a, x, cotangents, grad, tendencies); },
                                   [&](const Mp1mConsts<FT> &c, const A &a, auto FL) {
                                       launch<kProd1mBS>(vjp_kernel<Mp1mJac<decltype(FL)::value>, FT, K, kProd1mBS, Mp1mConsts<FT>>, n, s, c, a, n);
                                   });
}

}  // namespace cmx

extern "C" {
int32_t cmx_mp1m_jvp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho, const float *T,
                         const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                         const float *const tangents[CMX_MP1M_JAC_NWRT], float *const jvp[CMX_MP1M_JAC_NOUT], float *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream) {
    return cmx::jvp_1m_entry<float>(mp, tps, flags, n_points, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, tangents, jvp, tendencies, stream);
}
int32_t cmx_mp1m_jvp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho, const double *T,
                         const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                         const double *const tangents[CMX_MP1M_JAC_NWRT], double *const jvp[CMX_MP1M_JAC_NOUT], double *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream) {
    return cmx::jvp_1m_entry<double>(mp, tps, flags, n_points, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, tangents, jvp, tendencies, stream);
}
int32_t cmx_mp1m_vjp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho, const float *T,
                         const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                         const float *const cotangents[CMX_MP1M_JAC_NOUT], float *const grad[CMX_MP1M_JAC_NWRT], float *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream) {
    return cmx::vjp_1m_entry<float>(mp, tps, flags, n_points, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, cotangents, grad, tendencies, stream);
}
int32_t cmx_mp1m_vjp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho, const double *T,
                         const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                         const double *const cotangents[CMX_MP1M_JAC_NOUT], double *const grad[CMX_MP1M_JAC_NWRT], double *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream) {
    return cmx::vjp_1m_entry<double>(mp, tps, flags, n_points, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, cotangents, grad, tendencies, stream);
}
}
