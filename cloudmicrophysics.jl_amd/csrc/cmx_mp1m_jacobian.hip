// cmx_mp1m_jacobian.hip — the Jacobian of the 1-moment tendencies (BMT:141-252, 505-514) with respect to the state, over columns, for gfx950, and its
// products J v and Jᵀḡ; C-ABI entry points cmx_mp1m_jacobian_* / cmx_mp1m_jvp_* / cmx_mp1m_vjp_* / cmx_mp1m_implicit_tendencies_* / cmx_mp1m_implicit_average_* (include/cmx.h §(15), §(17), §(18), §(19)).  The SAME point function
// mp1m_point + mp1m_aggregate (cmx_mp1m.hpp) that the tendencies entry runs is instantiated on the forward-mode dual value type of cmx_dual.hpp — there is no
// second implementation of the physics and no finite difference; the donor-based linearization of LinearizedAverage (BMT:269-379) is an approximation and not
// this.
//
// Kernel shape (that of cmx_sb2006_jacobian.hip): one point per lane.  The seven input columns are read once; the point function is then evaluated
// ⌈n_seeded/K⌉ times inside the kernel, each pass carrying K tangents (K directions of the six inputs that can be differentiated; ρ is held fixed and its
// tangents are structural zeros).  Which input a tangent slot stands for, and which columns it is written to, is a small table in the kernel arguments
// (uniform loads), so one instantiation per float type and FLAGS serves every selection of columns, and a subset in any order computes, per column, exactly
// the instruction sequence of the full call.  Every pass recomputes the primal and every pass's primal is the plain instantiation's, bit for bit.  Stores
// are plain whole-column vector stores (one element per lane).  No LDS beyond the Float64 math tables every Float64 kernel of the library stages
// (cmx_lean_f64.hpp), no inline assembly here.  The kernel and the point's body are the shared driver's (jacobian_kernel<Mp1mJac<FLAGS>, …>, cmx_jacobian.hpp);
// the scheme it runs is shared with the host test build (cmx_mp1m_jacobian.hpp).
//
// FLAGS: the compile-time default-options / default-exponents instantiation or the run-time-flags one, chosen by flags_1m() as in cmx_mp1m_tendencies_*.
// K per float type (kJac1mK, cmx_mp1m_jacobian.hpp; kVjp1mK below, -DCMX_VJP1M_K_F32=…, -DCMX_VJP1M_K_F64=…: the Jacobian's by default) from the register
// counts of a cross-compiled build (tools/kernel_resources.py; DESIGN.md §9 has the table).  A translation unit of its own: no other kernel's code changes.
//
// The products (what they are for and their kernel shape: cmx_sb2006_jacobian.hip) run the same scheme through jvp_kernel / vjp_kernel.
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
constexpr int kJac1mBS = CMX_JAC1M_BS, kNOut = CMX_MP1M_JAC_NOUT, kNWrt = CMX_MP1M_JAC_NWRT;
template <typename FT> constexpr int kVjp1mK = sizeof(FT) == 4 ? CMX_VJP1M_K_F32 : CMX_VJP1M_K_F64;

// ---- host side -----------------------------------------------------------------------------------------------------
// The one entry of the three operations.  The statuses of the tendencies entry (tendencies_1m_entry, cmx_mp1m_kernels.hip), in its order; `table`: the
// tangent / cotangent table, which must not be NULL itself.
// make(a): fills the kernel's argument struct ARGS, false if the call has no output column at all.  kernel(S): the operation's kernel for the scheme S.
template <typename ARGS, typename FT, typename MP, typename TH, typename MAKE, typename KERNEL>
static int32_t entry(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], bool table, void *stream, MAKE &&make, KERNEL &&kernel) {
    if (!mp || !tps) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT_LIMIT(n);
    if (const int32_t st = check_flags_1m(flags)) return st;
    if (n == 0) return CMX_OK;
    for (const FT *p : in)
        if (!p) return CMX_ERR_BAD_ARG;
    ARGS a;
    if (!table || !make(a)) return CMX_ERR_BAD_ARG;
    return with_mp1m_jac<FT>(*mp, *tps, flags, [&](const Mp1mConsts<FT> &c, auto S) {
        // One point per lane with 4- / 8-byte accesses: any alignment and any n go through one launch (split_aligned with vec = 1 is the single range [0, n)
        // whatever the columns' addresses are, cmx_split.hpp)
        launch<kJac1mBS>(kernel(S), n, reinterpret_cast<hipStream_t>(stream), c, a, n);
        return launched();
    });
}

template <typename FT, typename MP, typename TH>
static int32_t jacobian_entry(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], FT *const *jac, FT *const *tendencies, void *stream) {
    using A = JacArgs<FT, kJac1mK<FT>, kNOut, kNWrt>;
    return entry<A>(mp, tps, flags, n, in, true, stream, [&](A &a) { return make_jac_args(a, in, jac, tendencies); },
                    [](auto S) { return jacobian_kernel<decltype(S), FT, kJac1mK<FT>, kJac1mBS, Mp1mConsts<FT>>; });
}

template <typename FT, typename MP, typename TH>
static int32_t jvp_entry(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], const FT *const *tangents, FT *const *jvp,
                         FT *const *tendencies, void *stream) {
    using A = JvpArgs<FT, kNOut, kNWrt>;
    return entry<A>(mp, tps, flags, n, in, tangents != nullptr, stream, [&](A &a) { return make_jvp_args(a, in, tangents, jvp, tendencies); },
                    [](auto S) { return jvp_kernel<decltype(S), FT, kJac1mBS, Mp1mConsts<FT>>; });
}

template <typename FT, typename MP, typename TH>
static int32_t vjp_entry(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], const FT *const *cotangents, FT *const *grad,
                         FT *const *tendencies, void *stream) {
    using A = VjpArgs<FT, kVjp1mK<FT>, kNOut, kNWrt>;
    return entry<A>(mp, tps, flags, n, in, cotangents != nullptr, stream, [&](A &a) { return make_vjp_args(a, in, cotangents, grad, tendencies); },
                    [](auto S) { return vjp_kernel<decltype(S), FT, kVjp1mK<FT>, kJac1mBS, Mp1mConsts<FT>>; });
}

// (I − Δt J)⁻¹ f (cmx_jacobian.hpp implicit_point; include/cmx.h §(18)).  `implicit` is the table: it must not be NULL itself; Δt is checked after the columns.
template <typename FT, typename MP, typename TH>
static int32_t implicit_entry(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], double dt, FT *const *implicit,
                              FT *const *tendencies, void *stream) {
    using A = ImplicitArgs<FT, kImplicitK<FT>, kNOut, kNWrt>;
    return entry<A>(mp, tps, flags, n, in, implicit != nullptr, stream,
                    [&](A &a) { return implicit_dt_ok(dt) && make_implicit_args(a, in, Mp1mJac<kDefaultFlags>::SPECIES0, dt, implicit, tendencies); },
                    [](auto S) { return implicit_kernel<decltype(S), FT, kImplicitK<FT>, kJac1mBS, Mp1mConsts<FT>>; });
}

// The average tendency over Δt from nsub implicit substeps (cmx_jacobian.hpp implicit_average_point; include/cmx.h §(19)).  `average` is the table: it must
// not be NULL itself; Δt, nsub and the step flags are checked after the columns.
template <typename FT, typename MP, typename TH>
static int32_t implicit_average_entry(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], double dt, int32_t nsub,
                                      uint32_t step_flags, FT *const *average, void *stream) {
    using A = ImplicitAverageArgs<FT, kImplicitAvgK<FT>, kNOut, kNWrt>;
    return entry<A>(mp, tps, flags, n, in, average != nullptr, stream,
                    [&](A &a) {
                        return implicit_average_step_ok<FT>(dt, nsub, step_flags) &&
                               make_implicit_average_args(a, in, Mp1mJac<kDefaultFlags>::SPECIES0, dt, nsub, step_flags, (FT)tps->LH_v0, (FT)tps->LH_s0, (FT)tps->cp_d, average);
                    },
                    [](auto S) { return implicit_average_kernel<decltype(S), FT, kImplicitAvgK<FT>, kJac1mBS, Mp1mConsts<FT>>; });
}

}  // namespace cmx

extern "C" {
int32_t cmx_mp1m_jacobian_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                              const float *T, const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                              float *const jac[CMX_MP1M_JAC_NCOL], float *const tendencies[CMX_MP1M_JAC_NOUT], void *stream) {
    return cmx::jacobian_entry<float>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, jac, tendencies, stream);
}
int32_t cmx_mp1m_jacobian_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                              const double *T, const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                              double *const jac[CMX_MP1M_JAC_NCOL], double *const tendencies[CMX_MP1M_JAC_NOUT], void *stream) {
    return cmx::jacobian_entry<double>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, jac, tendencies, stream);
}
int32_t cmx_mp1m_jvp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho, const float *T,
                         const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                         const float *const tangents[CMX_MP1M_JAC_NWRT], float *const jvp[CMX_MP1M_JAC_NOUT], float *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream) {
    return cmx::jvp_entry<float>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, tangents, jvp, tendencies, stream);
}
int32_t cmx_mp1m_jvp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho, const double *T,
                         const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                         const double *const tangents[CMX_MP1M_JAC_NWRT], double *const jvp[CMX_MP1M_JAC_NOUT], double *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream) {
    return cmx::jvp_entry<double>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, tangents, jvp, tendencies, stream);
}
int32_t cmx_mp1m_vjp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho, const float *T,
                         const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                         const float *const cotangents[CMX_MP1M_JAC_NOUT], float *const grad[CMX_MP1M_JAC_NWRT], float *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream) {
    return cmx::vjp_entry<float>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, cotangents, grad, tendencies, stream);
}
int32_t cmx_mp1m_vjp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho, const double *T,
                         const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                         const double *const cotangents[CMX_MP1M_JAC_NOUT], double *const grad[CMX_MP1M_JAC_NWRT], double *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream) {
    return cmx::vjp_entry<double>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, cotangents, grad, tendencies, stream);
}
int32_t cmx_mp1m_implicit_tendencies_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                         const float *T, const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                                         double dt, float *const implicit[CMX_MP1M_JAC_NOUT], float *const tendencies[CMX_MP1M_JAC_NOUT], void *stream) {
    return cmx::implicit_entry<float>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, dt, implicit, tendencies, stream);
}
int32_t cmx_mp1m_implicit_tendencies_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                         const double *T, const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                                         double dt, double *const implicit[CMX_MP1M_JAC_NOUT], double *const tendencies[CMX_MP1M_JAC_NOUT], void *stream) {
    return cmx::implicit_entry<double>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, dt, implicit, tendencies, stream);
}
int32_t cmx_mp1m_implicit_average_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                      const float *T, const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                                      double dt, int32_t nsub, uint32_t step_flags, float *const average[CMX_MP1M_JAC_NOUT], void *stream) {
    return cmx::implicit_average_entry<float>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, dt, nsub, step_flags, average, stream);
}
int32_t cmx_mp1m_implicit_average_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                      const double *T, const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                                      double dt, int32_t nsub, uint32_t step_flags, double *const average[CMX_MP1M_JAC_NOUT], void *stream) {
    return cmx::implicit_average_entry<double>(mp, tps, flags, n_points, {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, dt, nsub, step_flags, average, stream);
}
}
