// cmx_mp1m_jacobian.hpp — what the device entries (cmx_mp1m_jacobian.hip) and the host test build (tests/native/derivatives_host.cpp, CMX_HOST_BUILD) share
// of the 1-moment tendency Jacobian and its products: the tangents per pass, the scheme Mp1mJac that the driver of cmx_jacobian.hpp runs — the point function
// mp1m_point + mp1m_aggregate (cmx_mp1m.hpp) on the dual value type (cmx_dual.hpp) and the entry's poison rule — and its set-up from the parameter structs
// (with_mp1m_jac).  No HIP in here.
#pragma once
#include <cstdint>

#include "../../include/cmx.h"
#include "cmx_jacobian.hpp"
#include "cmx_mp1m.hpp"
#include "cmx_param_tangent.hpp"

namespace cmx {

// Tangents carried per evaluation of the point function, per float type: tuning numbers (-DCMX_JAC1M_K_F32=…, -DCMX_JAC1M_K_F64=…).  A pass costs one primal
// plus K tangent evaluations, so fewer, wider passes issue fewer instructions in all, as long as the kernel keeps its waves and spills nothing.  3 / 2 from
// the register counts (Float32 K = 3: 142–162 VGPRs, three waves per SIMD; Float64 K = 2: 226–276, K = 3: 272–338, K = 6 spills): the table of DESIGN.md §9;
// tools/time_jacobian.py --scheme mp1m times a build with another K (CMX_LIB).
#ifndef CMX_JAC1M_K_F32
#define CMX_JAC1M_K_F32 3
#endif
#ifndef CMX_JAC1M_K_F64
#define CMX_JAC1M_K_F64 2
#endif
template <typename FT> constexpr int kJac1mK = sizeof(FT) == 4 ? CMX_JAC1M_K_F32 : CMX_JAC1M_K_F64;

// The scheme (cmx_jacobian.hpp) of point x = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno): the four tendencies as duals.  The clamps of the inputs
// (BMT:147-152; T is not clamped) are the point function's own and so part of the differentiated function.  The value parts are mp1m_tendencies_point's
// results bit for bit (before its NaN rule, which is `out`).
template <uint32_t FLAGS> struct Mp1mJac {
    static constexpr int NOUT = CMX_MP1M_JAC_NOUT, NWRT = CMX_MP1M_JAC_NWRT;
    static constexpr int SPECIES0 = CMX_MP1M_JAC_WRT_Q_LCL;      // the first of the NOUT inputs whose tendencies the outputs are (implicit_point)
    static constexpr int TEMP = CMX_MP1M_JAC_WRT_T;               // the input that follows the latent heating of a substep (implicit_average_point)
    // the heating rate of the substep's rates d over c_p, the reference's expression (BMT:619-623; plain operations, no fma)
    template <typename FT> static __device__ __forceinline__ FT heating(FT Lv, FT Ls, const FT (&d)[NOUT]) {
        return Lv * (d[CMX_MP1M_JAC_DQ_LCL_DT] + d[CMX_MP1M_JAC_DQ_RAI_DT]) + Ls * (d[CMX_MP1M_JAC_DQ_ICL_DT] + d[CMX_MP1M_JAC_DQ_SNO_DT]);
    }
    // the poison rule of the 1-moment entries (mp1m_tendencies_point): a NaN in any input column — in Float64 also ρ ≤ 0 (cmx_math.hpp bad_density) — gives NaN
    // in every output of the point.  A select, not SB2006's sum: −0 stays −0
    template <typename FT> static __device__ __forceinline__ bool poison(const FT (&x)[NWRT + 1]) {
        return (bool)((int)any_nan(x[0], x[2], x[3], x[4], x[5], x[6], x[1]) | (int)bad_density(x[0]));
    }
    template <typename FT> static __device__ __forceinline__ FT out(FT v, bool bad) { return bad ? Math<FT>::nan() : v; }
    // in: the six differentiated inputs in the order of cmx_mp1m_jac_wrt.  `c` is the kernel's constants argument: Float64 (and the run-time-flags Float32
    // instantiation) reads it through the kernel-argument segment, phase by phase (cmx_math.hpp front_consts)
    template <typename FT, int K, typename C>
    static __device__ __forceinline__ void eval(const C &c, FT rho, const Dual<FT, K> (&in)[NWRT], Dual<FT, K> (&o)[NOUT]) {
        using D = Dual<FT, K>;
        const Mp1mSrc<D> p = mp1m_point<D, FLAGS>(scheme_consts<FT, FLAGS == kRuntimeFlags>(c), D(rho), in[CMX_MP1M_JAC_WRT_T], in[CMX_MP1M_JAC_WRT_Q_TOT],
                                                  in[CMX_MP1M_JAC_WRT_Q_LCL], in[CMX_MP1M_JAC_WRT_Q_ICL], in[CMX_MP1M_JAC_WRT_Q_RAI], in[CMX_MP1M_JAC_WRT_Q_SNO]);
        mp1m_aggregate<D>(p, o[CMX_MP1M_JAC_DQ_LCL_DT], o[CMX_MP1M_JAC_DQ_ICL_DT], o[CMX_MP1M_JAC_DQ_RAI_DT], o[CMX_MP1M_JAC_DQ_SNO_DT]);
    }
};

// The set-up every 1-moment derivative entry and its host mirror share after the argument checks (check_flags_1m among them: it comes earlier in the
// entries' status order): the constants and the instantiation flags_1m chooses as in cmx_mp1m_tendencies_*.  Returns f(c, Mp1mJac<FLAGS>{}).
template <typename FT, typename MP, typename TH, typename F> inline int32_t with_mp1m_jac(const MP &mp, const TH &tps, uint32_t flags, F &&f) {
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(mp, tps, flags, (double)Math<FT>::eps_1m());
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto FL) -> int32_t { return f(c, Mp1mJac<decltype(FL)::value>{}); }, flags_1m(flags, c));
}

// ---- ∂/∂θ (cmx_jacobian.hpp param_jvp_point / param_vjp_point; include/cmx.h §(23)) ------------------------------------------------------------------------------
// The fold of one direction on ParamTan, and the constants of ONE launch: tangent slot k holds ċ of direction d0 + k (an idle slot past ndir: zeros).  Every
// slot's value parts are the same, and the plain fold's, bit for bit.
template <typename FT, typename MP, typename TH>
inline Mp1mConsts<ParamTan> make_mp1m_tangent_consts(const MP &mp, const TH &tps, uint32_t flags, const MP *d_mp, const TH *d_tps) {
    return make_mp1m_consts_from<FT, ParamTan>(mp, tps, flags, (double)Math<FT>::eps_1m(), ParamReader<MP>{mp, d_mp}, ParamReader<TH>{tps, d_tps});
}
template <typename FT, int KP, typename MP, typename TH>
inline Mp1mConsts<Dual<FT, KP>> make_mp1m_param_consts(const MP &mp, const TH &tps, uint32_t flags, const MP *d_mp, const TH *d_tps, int d0, int ndir) {
    Mp1mConsts<Dual<FT, KP>> cd{};
    cd.flags = flags;
    for (int k = 0; k < KP; ++k) {
        const bool live = d0 + k < ndir;
        const Mp1mConsts<ParamTan> ct = make_mp1m_tangent_consts<FT>(mp, tps, flags, live ? d_mp + d0 + k : nullptr, live && d_tps ? d_tps + d0 + k : nullptr);
        pack_param_members<KP>(ct, &ct.eps_1m, k, cd, &cd.eps_1m);
    }
    return cd;
}
static_assert(sizeof(Mp1mConsts<Dual<float, kParamK<float>>>) + 512 <= 4096 && sizeof(Mp1mConsts<Dual<double, kParamK<double>>>) + 512 <= 4096,
              "CMX_PARAM_K_F32 / CMX_PARAM_K_F64: the constants with their tangents must fit the 4 KiB kernel-argument segment");

// The checks of the directions and the instantiation choice, after the entry's own argument checks (check_flags_1m among them).  The default-options
// instantiation holds the nine slope-parameter exponents of mp1m_default_exponents as compile-time numbers and so has no derivative with respect to them: it
// runs only if the tendencies entry would select it AND no direction gives one of the nine a non-zero tangent; otherwise the run-time-flags instantiation runs
// for the whole call.  Returns f(Mp1mJac<FLAGS>{}) or CMX_ERR_BAD_ARG.
template <typename FT, typename MP, typename TH, typename F>
inline int32_t with_mp1m_param(const MP &mp, const TH &tps, uint32_t flags, int32_t ndir, const MP *d_mp, const TH *d_tps, F &&f) {
    if (ndir < 1 || ndir > CMX_PARAM_MAX_DIRS || !d_mp) return CMX_ERR_BAD_ARG;
    bool exponents = false;
    for (int d = 0; d < ndir; ++d) {
        if (!all_finite<FT>(d_mp[d]) || (d_tps && !all_finite<FT>(d_tps[d]))) return CMX_ERR_BAD_ARG;
        const Mp1mConsts<ParamTan> t = make_mp1m_tangent_consts<FT>(mp, tps, flags, d_mp + d, d_tps ? d_tps + d : nullptr);
        for (const ParamTan &e : {t.vt_e_rai, t.acc_e_rai, t.sink_e, t.rs_dp1_rai, t.ven_e_rai, t.vt_e_sno, t.acc_e_sno, t.rs_dp1_sno, t.ven_e_sno}) exponents |= e.d != 0;
    }
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(mp, tps, flags, (double)Math<FT>::eps_1m());
    const bool fast = flags == CMX_1M_DEFAULT_OPTIONS && mp1m_default_exponents(c) && !exponents;
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto FL) -> int32_t { return f(Mp1mJac<decltype(FL)::value>{}); },
                       one_of<kDefaultFlags, kRuntimeFlags>(fast ? kDefaultFlags : kRuntimeFlags));
}

}  // namespace cmx
