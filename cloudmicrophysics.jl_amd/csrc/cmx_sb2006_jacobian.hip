// cmx_sb2006_jacobian.hip — the Jacobian of the SB2006 warm-rain tendencies (BMT:707-782, 820-854) with respect to the prognostic state, over columns, for
// gfx950; C-ABI entry points cmx_sb2006_warm_rain_jacobian_* (include/cmx.h §(14)).  The reference differentiates bulk_microphysics_tendencies with
// ForwardDiff (test/ad_compat_tests.jl:106-175); here the SAME point function sb2006_point (cmx_sb2006.hpp) is instantiated on the forward-mode dual value
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
// K per float type (kJacK, cmx_sb2006_jacobian.hpp) from the register counts of a cross-compiled build (tools/kernel_resources.py; DESIGN.md §9 has the table).
// A translation unit of its own: no existing kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_sb2006_jacobian.hpp"

namespace cmx {

#ifndef CMX_JAC_BS
#define CMX_JAC_BS 256
#endif
constexpr int kJacBS = CMX_JAC_BS;

// ---- host side -----------------------------------------------------------------------------------------------------
template <typename FT, typename WR, typename TH>
static int32_t jacobian_entry(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *rho, const FT *T, const FT *q_tot, const FT *q_lcl,
                              const FT *n_lcl, const FT *q_rai, const FT *n_rai, FT *const *jac, FT *const *tendencies, void *stream) {
    // the statuses of the tendencies entry, in its order: parameters, the count rule, the columns, the flags, the limiters
    if (!wr || !tps) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT(n);
    if (!rho || !T || !q_tot || !q_lcl || !n_lcl || !q_rai || !n_rai) return CMX_ERR_BAD_ARG;
    constexpr int K = kJacK<FT>;
    SbJacArgs<FT, K> a;
    const FT *const in[7] = {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai};
    if (!make_jac_args(a, in, jac, tendencies)) return CMX_ERR_BAD_ARG;      // no output column at all
    if (flags & ~(uint32_t)CMX_SB2006_LIMITED) return CMX_ERR_BAD_ARG;
    const bool limited = flags & CMX_SB2006_LIMITED;
    if (limited && !sb_limiters_ok(*wr)) return CMX_ERR_BAD_ARG;      // clamp_ordered needs ordered limiter pairs
    const SbConsts<FT> c = make_sb_consts<FT>(*wr, *tps, (const std::conditional_t<std::is_same_v<FT, float>, cmx_rain_vel_f32, cmx_rain_vel_f64> *)nullptr,
                                              (double)Math<FT>::eps_1m());
    const bool intpow = sb_integer_exponents(*wr);        // the instantiation the tendencies entry selects for the same parameter struct
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // One point per lane with 4- / 8-byte accesses: any alignment and any n go through one launch.  (The alignment split of the vector kernels is the
    // identity here: split_aligned with vec = 1 is the single scalar range [0, n) whatever the columns' addresses are, cmx_split.hpp.)
    dispatch([&](auto L, auto I) {
        launch<kJacBS>(jacobian_kernel<SbJac<decltype(L)::value, decltype(I)::value>, FT, K, kJacBS, SbConsts<FT>>, n, s, c, a, n);
    }, flag(limited), flag(intpow));
    return launched();
}

}  // namespace cmx

extern "C" {
int32_t cmx_sb2006_warm_rain_jacobian_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                          const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                          float *const jac[CMX_SB2006_JAC_NCOL], float *const tendencies[CMX_SB2006_JAC_NOUT],
                                          void *stream) {
    return cmx::jacobian_entry<float>(warm_rain, tps, flags, n_points, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, jac, tendencies, stream);
}
int32_t cmx_sb2006_warm_rain_jacobian_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                          const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                          const double *n_rai, double *const jac[CMX_SB2006_JAC_NCOL],
                                          double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream) {
    return cmx::jacobian_entry<double>(warm_rain, tps, flags, n_points, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, jac, tendencies, stream);
}
}
