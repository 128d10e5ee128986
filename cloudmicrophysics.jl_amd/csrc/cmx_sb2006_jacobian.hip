// cmx_sb2006_jacobian.hip — the Jacobian of the SB2006 warm-rain tendencies (BMT:707-782, 820-854) with respect to the prognostic state, over columns, for
// gfx950, and its products J v and Jᵀḡ; C-ABI entry points cmx_sb2006_warm_rain_jacobian_* / _jvp_* / _vjp_* / _implicit_tendencies_* / _implicit_average_* (include/cmx.h §(14), §(16), §(18), §(19)).  The reference
// differentiates bulk_microphysics_tendencies with ForwardDiff (test/ad_compat_tests.jl:106-175); here the SAME point function sb2006_point (cmx_sb2006.hpp) is instantiated on the forward-mode dual value
// type of cmx_dual.hpp — there is no second implementation of the physics and no finite difference.
//
// Kernel shape: one point per lane.  The seven input columns are read once; the point function is then evaluated ⌈n_seeded/K⌉ times inside the kernel, each
// pass carrying K tangents (K directions of the six inputs that can be differentiated; ρ is held fixed and its tangents are structural zeros).  Which input a
// tangent slot stands for, and which columns it is written to, is a small table in the kernel arguments (uniform loads), so one instantiation per float type,
// LIMITED and INTPOW serves every selection of columns, and a subset in any order computes, per column, exactly the instruction sequence of the full call.
// Every pass recomputes the primal — that is what forward mode costs — and every pass's primal is the plain instantiation's, bit for bit.  Stores are plain
// whole-column vector stores (one element per lane, a wave writes 256 / 512 contiguous bytes).  No LDS beyond the Float64 math tables every Float64 kernel
// of the library stages (cmx_lean_f64.hpp), no inline assembly here.  The kernel and the point's body are the shared driver's (jacobian_kernel<SbJac<…>, …>,
// cmx_jacobian.hpp); the scheme it runs is shared with the host test build (cmx_sb2006_jacobian.hpp).
//
// The products are what a Jacobian-free Newton–Krylov matvec and a gradient (torch autograd, cmx/autograd.py) consume: 4 resp. 6 columns out instead of the
// 24 of the Jacobian and a second pass that contracts them.  Same scheme, same kernel shape (jvp_kernel / vjp_kernel): J v is ONE evaluation on Dual<FT, 1>
// seeded with the caller's tangent, Jᵀḡ is ⌈n_grad/K⌉ evaluations on Dual<FT, K> with unit seeds whose tangents are contracted with the cotangents in registers.
//
// K per float type (kJacK, cmx_sb2006_jacobian.hpp; kVjpK below, -DCMX_VJP_K_F32=…, -DCMX_VJP_K_F64=…: the Jacobian's by default) from the register counts of
// a cross-compiled build (tools/kernel_resources.py; DESIGN.md §9 has the table).  A translation unit of its own: no other kernel's code changes.
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
constexpr int kJacBS = CMX_JAC_BS, kNOut = CMX_SB2006_JAC_NOUT, kNWrt = CMX_SB2006_JAC_NWRT;
template <typename FT> constexpr int kVjpK = sizeof(FT) == 4 ? CMX_VJP_K_F32 : CMX_VJP_K_F64;

// ---- host side -----------------------------------------------------------------------------------------------------
// The one entry of the three operations.  The statuses of the tendencies entry, in its order: parameters, the count rule, the columns, [`table`: the
// tangent / cotangent table, which must not be NULL itself,] no output column at all, the flags, the limiters.
// make(a): fills the kernel's argument struct ARGS, false if the call has no output column at all.  kernel(S): the operation's kernel for the scheme S.
template <typename ARGS, typename FT, typename WR, typename TH, typename MAKE, typename KERNEL>
static int32_t entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], bool table, void *stream, MAKE &&make, KERNEL &&kernel) {
    if (!wr || !tps) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT(n);
    for (const FT *p : in)
        if (!p) return CMX_ERR_BAD_ARG;
    ARGS a;
    if (!table || !make(a)) return CMX_ERR_BAD_ARG;
    return with_sb2006_jac<FT>(*wr, *tps, flags, [&](const SbConsts<FT> &c, auto S) {
        // One point per lane with 4- / 8-byte accesses: any alignment and any n go through one launch.  (The alignment split of the vector kernels is the
        // identity here: split_aligned with vec = 1 is the single scalar range [0, n) whatever the columns' addresses are, cmx_split.hpp.)
        launch<kJacBS>(kernel(S), n, reinterpret_cast<hipStream_t>(stream), c, a, n);
        return launched();
    });
}

template <typename FT, typename WR, typename TH>
static int32_t jacobian_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], FT *const *jac, FT *const *tendencies, void *stream) {
    using A = JacArgs<FT, kJacK<FT>, kNOut, kNWrt>;
    return entry<A>(wr, tps, flags, n, in, true, stream, [&](A &a) { return make_jac_args(a, in, jac, tendencies); },
                    [](auto S) { return jacobian_kernel<decltype(S), FT, kJacK<FT>, kJacBS, SbConsts<FT>>; });
}

template <typename FT, typename WR, typename TH>
static int32_t jvp_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], const FT *const *tangents, FT *const *jvp,
                         FT *const *tendencies, void *stream) {
    using A = JvpArgs<FT, kNOut, kNWrt>;
    return entry<A>(wr, tps, flags, n, in, tangents != nullptr, stream, [&](A &a) { return make_jvp_args(a, in, tangents, jvp, tendencies); },
                    [](auto S) { return jvp_kernel<decltype(S), FT, kJacBS, SbConsts<FT>>; });
}

template <typename FT, typename WR, typename TH>
static int32_t vjp_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], const FT *const *cotangents, FT *const *grad,
                         FT *const *tendencies, void *stream) {
    using A = VjpArgs<FT, kVjpK<FT>, kNOut, kNWrt>;
    return entry<A>(wr, tps, flags, n, in, cotangents != nullptr, stream, [&](A &a) { return make_vjp_args(a, in, cotangents, grad, tendencies); },
                    [](auto S) { return vjp_kernel<decltype(S), FT, kVjpK<FT>, kJacBS, SbConsts<FT>>; });
}

// (I − Δt J)⁻¹ f (cmx_jacobian.hpp implicit_point; include/cmx.h §(18)).  `implicit` is the table: it must not be NULL itself; Δt is checked after the columns.
template <typename FT, typename WR, typename TH>
static int32_t implicit_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], double dt, FT *const *implicit,
                              FT *const *tendencies, void *stream) {
    using A = ImplicitArgs<FT, kImplicitK<FT>, kNOut, kNWrt>;
    return entry<A>(wr, tps, flags, n, in, implicit != nullptr, stream,
                    [&](A &a) { return implicit_dt_ok(dt) && make_implicit_args(a, in, SbJac<false, false>::SPECIES0, dt, implicit, tendencies); },
                    [](auto S) { return implicit_kernel<decltype(S), FT, kImplicitK<FT>, kJacBS, SbConsts<FT>>; });
}

// The average tendency over Δt from nsub implicit substeps (cmx_jacobian.hpp implicit_average_point; include/cmx.h §(19)).  `average` is the table: it must
// not be NULL itself; Δt, nsub and the step flags are checked after the columns.
template <typename FT, typename WR, typename TH>
static int32_t implicit_average_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const (&in)[7], double dt, int32_t nsub,
                                      uint32_t step_flags, FT *const *average, void *stream) {
    using A = ImplicitAverageArgs<FT, kImplicitAvgK<FT>, kNOut, kNWrt>;
    return entry<A>(wr, tps, flags, n, in, average != nullptr, stream,
                    [&](A &a) {
                        return implicit_average_step_ok<FT>(dt, nsub, step_flags) &&
                               make_implicit_average_args(a, in, SbJac<false, false>::SPECIES0, dt, nsub, step_flags, (FT)tps->LH_v0, (FT)tps->LH_s0, (FT)tps->cp_d, average);
                    },
                    [](auto S) { return implicit_average_kernel<decltype(S), FT, kImplicitAvgK<FT>, kJacBS, SbConsts<FT>>; });
}

}  // namespace cmx

extern "C" {
int32_t cmx_sb2006_warm_rain_jacobian_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                          const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                          float *const jac[CMX_SB2006_JAC_NCOL], float *const tendencies[CMX_SB2006_JAC_NOUT],
                                          void *stream) {
    return cmx::jacobian_entry<float>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, jac, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_jacobian_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                          const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                          const double *n_rai, double *const jac[CMX_SB2006_JAC_NCOL],
                                          double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::jacobian_entry<double>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, jac, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_jvp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                     const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                     const float *const tangents[CMX_SB2006_JAC_NWRT], float *const jvp[CMX_SB2006_JAC_NOUT],
                                     float *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::jvp_entry<float>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, tangents, jvp, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_jvp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                     const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai,
                                     const double *const tangents[CMX_SB2006_JAC_NWRT], double *const jvp[CMX_SB2006_JAC_NOUT],
                                     double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::jvp_entry<double>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, tangents, jvp, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_vjp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                     const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                     const float *const cotangents[CMX_SB2006_JAC_NOUT], float *const grad[CMX_SB2006_JAC_NWRT],
                                     float *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::vjp_entry<float>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, cotangents, grad, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_vjp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                     const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai,
                                     const double *const cotangents[CMX_SB2006_JAC_NOUT], double *const grad[CMX_SB2006_JAC_NWRT],
                                     double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::vjp_entry<double>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, cotangents, grad, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_implicit_tendencies_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points,
                                                     const float *rho, const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl,
                                                     const float *q_rai, const float *n_rai, double dt, float *const implicit[CMX_SB2006_JAC_NOUT],
                                                     float *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::implicit_entry<float>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, dt, implicit, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_implicit_tendencies_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points,
                                                     const double *rho, const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl,
                                                     const double *q_rai, const double *n_rai, double dt, double *const implicit[CMX_SB2006_JAC_NOUT],
                                                     double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::implicit_entry<double>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, dt, implicit, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_implicit_average_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points,
                                                  const float *rho, const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl,
                                                  const float *q_rai, const float *n_rai, double dt, int32_t nsub, uint32_t step_flags,
                                                  float *const average[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::implicit_average_entry<float>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, dt, nsub, step_flags, average, stream);
}
int32_t cmx_sb2006_warm_rain_implicit_average_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points,
                                                  const double *rho, const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl,
                                                  const double *q_rai, const double *n_rai, double dt, int32_t nsub, uint32_t step_flags,
                                                  double *const average[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::implicit_average_entry<double>(warm_rain, tps, flags, n_points, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, dt, nsub, step_flags, average, stream);
}
}
