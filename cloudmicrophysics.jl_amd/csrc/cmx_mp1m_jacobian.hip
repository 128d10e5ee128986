// cmx_mp1m_jacobian.hip — the Jacobian of the 1-moment tendencies (BMT:141-252, 505-514) with respect to the state, over columns, for gfx950; C-ABI entry
// points cmx_mp1m_jacobian_* (include/cmx.h §(15)).  The SAME point function mp1m_point + mp1m_aggregate (cmx_mp1m.hpp) that the tendencies entry runs is
// instantiated on the forward-mode dual value type of cmx_dual.hpp — there is no second implementation of the physics and no finite difference; the
// donor-based linearization of LinearizedAverage (BMT:269-379) is an approximation and not this.
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
// K per float type (kJac1mK, cmx_mp1m_jacobian.hpp) from the register counts of a cross-compiled build (tools/kernel_resources.py; DESIGN.md §9 has the
// table).  A translation unit of its own: no existing kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_mp1m_jacobian.hpp"

namespace cmx {

#ifndef CMX_JAC1M_BS
#define CMX_JAC1M_BS 256
#endif
constexpr int kJac1mBS = CMX_JAC1M_BS;

// ---- host side -----------------------------------------------------------------------------------------------------
template <typename FT, typename MP, typename TH>
static int32_t jacobian_1m_entry(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *rho, const FT *T, const FT *q_tot, const FT *q_lcl,
                                 const FT *q_icl, const FT *q_rai, const FT *q_sno, FT *const *jac, FT *const *tendencies, void *stream) {
    // the statuses of the tendencies entry (tendencies_1m_entry, cmx_mp1m_kernels.hip), in its order
    if (!mp || !tps) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT_LIMIT(n);
    if (const int32_t st = check_flags_1m(flags)) return st;
    if (n == 0) return CMX_OK;
    if (!rho || !T || !q_tot || !q_lcl || !q_icl || !q_rai || !q_sno) return CMX_ERR_BAD_ARG;
    constexpr int K = kJac1mK<FT>;
    Mp1mJacArgs<FT, K> a;
    const FT *const in[7] = {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno};
    if (!make_jac_args(a, in, jac, tendencies)) return CMX_ERR_BAD_ARG;      // no output column at all
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(*mp, *tps, flags, (double)Math<FT>::eps_1m());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // One point per lane with 4- / 8-byte accesses: any alignment and any n go through one launch (split_aligned with vec = 1 is the single range [0, n)
    // whatever the columns' addresses are, cmx_split.hpp)
    dispatch([&](auto FL) { launch<kJac1mBS>(jacobian_kernel<Mp1mJac<decltype(FL)::value>, FT, K, kJac1mBS, Mp1mConsts<FT>>, n, s, c, a, n); }, flags_1m(flags, c));
    return launched();
}

}  // namespace cmx

extern "C" {
int32_t cmx_mp1m_jacobian_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                              const float *T, const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                              float *const jac[CMX_MP1M_JAC_NCOL], float *const tendencies[CMX_MP1M_JAC_NOUT], void *stream) {
    return cmx::jacobian_1m_entry<float>(mp, tps, flags, n_points, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, jac, tendencies, stream);
}
int32_t cmx_mp1m_jacobian_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                              const double *T, const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                              double *const jac[CMX_MP1M_JAC_NCOL], double *const tendencies[CMX_MP1M_JAC_NOUT], void *stream) {
    return cmx::jacobian_1m_entry<double>(mp, tps, flags, n_points, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, jac, tendencies, stream);
}
}
