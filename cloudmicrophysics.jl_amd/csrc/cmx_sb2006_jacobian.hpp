// cmx_sb2006_jacobian.hpp — what the device entries (cmx_sb2006_jacobian.hip) and the host test build (tests/native/derivatives_host.cpp, CMX_HOST_BUILD)
// share of the SB2006 warm-rain Jacobian and its products: the tangents per pass, the scheme SbJac that the driver of cmx_jacobian.hpp runs — the point function
// sb2006_point on the dual value type (cmx_dual.hpp) and the entry's NaN rule — and its set-up from the parameter structs (with_sb2006_jac).  No HIP in here.
#pragma once
#include <cstdint>
#include <type_traits>

#include "../../include/cmx.h"
#include "cmx_dispatch.hpp"
#include "cmx_jacobian.hpp"
#include "cmx_param_tangent.hpp"
#include "cmx_sb2006.hpp"

namespace cmx {

// Tangents carried per evaluation of the point function, per float type: tuning numbers (-DCMX_JAC_K_F32=…, -DCMX_JAC_K_F64=…).  A pass costs one primal plus
// K tangent evaluations, so fewer, wider passes issue fewer instructions in all, as long as the kernel keeps its waves.  3 in both types: Float32 stays
// inside 128 VGPRs (four waves per SIMD), Float64 runs at one wave per SIMD from K = 2 on and K = 3 is two passes for all six inputs and one for up to three.
// The registers and measured times of K = 1, 2, 3, 6 are the table of DESIGN.md §9.
#ifndef CMX_JAC_K_F32
#define CMX_JAC_K_F32 3
#endif
#ifndef CMX_JAC_K_F64
#define CMX_JAC_K_F64 3
#endif
template <typename FT> constexpr int kJacK = sizeof(FT) == 4 ? CMX_JAC_K_F32 : CMX_JAC_K_F64;

// The scheme (cmx_jacobian.hpp) of point x = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai): the four tendencies as duals.  The clamps, N = ρ n and the sums
// are sb2006_tendencies_kernel's (cmx_sb2006_kernels.hpp), so the value parts are that kernel's results bit for bit.
template <bool LIMITED, bool INTPOW> struct SbJac {
    static constexpr int NOUT = CMX_SB2006_JAC_NOUT, NWRT = CMX_SB2006_JAC_NWRT;
    static constexpr int SPECIES0 = CMX_SB2006_JAC_WRT_Q_LCL;      // the first of the NOUT inputs whose tendencies the outputs are (implicit_point)
    static constexpr int TEMP = CMX_SB2006_JAC_WRT_T;               // the input that follows the latent heating of a substep (implicit_average_point)
    // the heating rate of the substep's rates d over c_p: condensate formed from vapour, liquid only (plain operations, no fma)
    template <typename FT> static __device__ __forceinline__ FT heating(FT Lv, FT, const FT (&d)[NOUT]) {
        return Lv * (d[CMX_SB2006_JAC_DQ_LCL_DT] + d[CMX_SB2006_JAC_DQ_RAI_DT]);
    }
    // a NaN in any input column poisons every output of the point (cmx_math.hpp any_nan): x + NaN = NaN, x + 0 = x
    template <typename FT> static __device__ __forceinline__ FT poison(const FT (&x)[NWRT + 1]) {
        return any_nan(x[0], x[2], x[3], x[4], x[5], x[6], x[1]) ? Math<FT>::nan() : FT(0);
    }
    template <typename FT> static __device__ __forceinline__ FT out(FT v, FT poison) { return v + poison; }
    // in: the six differentiated inputs in the order of cmx_sb2006_jac_wrt
    template <typename FT, int K, typename C>
    static __device__ __forceinline__ void eval(const C &c, FT rho, const Dual<FT, K> (&in)[NWRT], Dual<FT, K> (&o)[NOUT]) {
        using D = Dual<FT, K>;
        using MD = Math<D>;
        // clamp_to_nonneg — BMT:828-837 (T is not clamped); the clamps are part of the differentiated function.  ρ is a constant: not differentiated
        const D r_ = D(max0(rho));
        const D T = in[CMX_SB2006_JAC_WRT_T];
        const D qt = max0(in[CMX_SB2006_JAC_WRT_Q_TOT]), ql = max0(in[CMX_SB2006_JAC_WRT_Q_LCL]), nl = max0(in[CMX_SB2006_JAC_WRT_N_LCL]);
        const D qr = max0(in[CMX_SB2006_JAC_WRT_Q_RAI]), nr = max0(in[CMX_SB2006_JAC_WRT_N_RAI]);
        // N = ρ n — BMT:718-719.  `c` is the kernel's constants argument: Float64 reads it through the kernel-argument segment, phase by phase
        // (cmx_math.hpp front_consts; constants that are duals themselves: the plain reference, cmx_dual.hpp scheme_consts)
        const SbRates<D> p = sb2006_point<D, LIMITED, VEL_NONE, false, INTPOW>(scheme_consts<FT>(c), r_, T, qt, ql, qr, r_ * nl, r_ * nr, nl, nr);
        o[CMX_SB2006_JAC_DQ_LCL_DT] = (p.cond + p.au_dq_lcl) + p.ac_dq_lcl;
        o[CMX_SB2006_JAC_DN_LCL_DT] = MD::fma(p.lsc_plus_au + p.ac_dN_lcl, p.inv_rho, p.na_lcl);
        o[CMX_SB2006_JAC_DQ_RAI_DT] = (p.evq + p.au_dq_rai) + p.ac_dq_rai;
        o[CMX_SB2006_JAC_DN_RAI_DT] = MD::fma(((p.evN + p.au_dN_rai) + p.rsc) + p.rbr, p.inv_rho, p.na_rai);
    }
};

// The set-up every SB2006 derivative entry and its host mirror share after the argument checks: the statuses of the flags and the limiter pairs, the constants,
// and the instantiation the tendencies entry selects for the same parameter struct.  Returns f(c, SbJac<LIMITED, INTPOW>{}) or CMX_ERR_BAD_ARG.
template <typename FT, typename WR, typename TH, typename F> inline int32_t with_sb2006_jac(const WR &wr, const TH &tps, uint32_t flags, F &&f) {
    if (flags & ~(uint32_t)CMX_SB2006_LIMITED) return CMX_ERR_BAD_ARG;
    const bool limited = flags & CMX_SB2006_LIMITED;
    if (limited && !sb_limiters_ok(wr)) return CMX_ERR_BAD_ARG;      // clamp_ordered needs ordered limiter pairs
    const SbConsts<FT> c = make_sb_consts<FT>(wr, tps, (const std::conditional_t<std::is_same_v<FT, float>, cmx_rain_vel_f32, cmx_rain_vel_f64> *)nullptr,
                                              (double)Math<FT>::eps_1m());
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto L, auto I) -> int32_t { return f(c, SbJac<decltype(L)::value, decltype(I)::value>{}); },
                       flag(limited), flag(sb_integer_exponents(wr)));
}

// ---- ∂/∂θ (cmx_jacobian.hpp param_jvp_point / param_vjp_point; include/cmx.h §(22)) ------------------------------------------------------------------------------
// The constants of ONE launch: tangent slot k holds ċ of direction d0 + k (an idle slot past ndir: zeros), from the fold of make_sb_consts_from on ParamTan.
// Every slot's value parts are the same, and the plain fold's, bit for bit.
template <typename FT, int KP, typename WR, typename TH>
inline SbConsts<Dual<FT, KP>> make_sb_param_consts(const WR &wr, const TH &tps, const WR *d_wr, const TH *d_tps, int d0, int ndir) {
    using VL = std::conditional_t<std::is_same_v<FT, float>, cmx_rain_vel_f32, cmx_rain_vel_f64>;
    SbConsts<Dual<FT, KP>> cd{};
    for (int k = 0; k < KP; ++k) {
        const bool live = d0 + k < ndir;
        const SbConsts<ParamTan> ct = make_sb_consts_from<FT, ParamTan>(wr, tps, (const VL *)nullptr, (double)Math<FT>::eps_1m(),
                                                                        ParamReader<WR>{wr, live ? d_wr + d0 + k : nullptr},
                                                                        ParamReader<TH>{tps, live && d_tps ? d_tps + d0 + k : nullptr});
        pack_param_consts<KP>(ct, k, cd);
    }
    return cd;
}
// the kernel-argument segment holds the dual constants next to the column tables
static_assert(sizeof(SbConsts<Dual<float, kParamK<float>>>) + 512 <= 4096 && sizeof(SbConsts<Dual<double, kParamK<double>>>) + 512 <= 4096,
              "CMX_PARAM_K_F32 / CMX_PARAM_K_F64: the constants with their tangents must fit the 4 KiB kernel-argument segment");

// The checks of the directions and the instantiation choice, after the entry's own argument checks: 1 ≤ ndir ≤ CMX_PARAM_MAX_DIRS, the table, finite
// components, then the flags and limiters of with_sb2006_jac.  The integer-exponent instantiation has no derivative with respect to acnv.b, accr.c, self.d:
// it runs only if the tendencies entry would select it AND no direction moves one of the three.  Returns f(SbJac<LIMITED, INTPOW>{}) or CMX_ERR_BAD_ARG.
template <typename FT, typename WR, typename TH, typename F>
inline int32_t with_sb2006_param(const WR &wr, const TH &tps, uint32_t flags, int32_t ndir, const WR *d_wr, const TH *d_tps, F &&f) {
    if (ndir < 1 || ndir > CMX_PARAM_MAX_DIRS || !d_wr) return CMX_ERR_BAD_ARG;
    bool exponents = false;
    for (int d = 0; d < ndir; ++d) {
        if (!all_finite<FT>(d_wr[d]) || (d_tps && !all_finite<FT>(d_tps[d]))) return CMX_ERR_BAD_ARG;
        const auto &sb = d_wr[d].seifert_beheng;
        exponents |= sb.acnv.b != 0 || sb.accr.c != 0 || sb.self.d != 0;
    }
    if (flags & ~(uint32_t)CMX_SB2006_LIMITED) return CMX_ERR_BAD_ARG;
    const bool limited = flags & CMX_SB2006_LIMITED;
    if (limited && !sb_limiters_ok(wr)) return CMX_ERR_BAD_ARG;
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto L, auto I) -> int32_t { return f(SbJac<decltype(L)::value, decltype(I)::value>{}); },
                       flag(limited), flag(sb_integer_exponents(wr) && !exponents));
}

}  // namespace cmx
