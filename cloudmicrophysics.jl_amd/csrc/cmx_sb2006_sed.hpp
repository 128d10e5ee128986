// cmx_sb2006_sed.hpp — the sedimentation fluxes of the SB2006 falling species, per point: what the fused column step (cmx_sb2006_column.hip) and the
// column step with the implicit average as tendency (cmx_column_implicit_average.hip) share, so that both form a flux with the same operations.
#pragma once
#include "cmx_sb2006.hpp"

namespace cmx {

template <typename FT> struct SedFlux { FT q_rai, n_rai, q_lcl, n_lcl; };

// fluxes of one (clamped) point from its fall speeds
template <typename FT, bool CLOUD, typename CV>      // FT: the value type (a point or a packed pair); CV: CloudVelConsts of its scalar type
__device__ __forceinline__ SedFlux<FT> sed_fluxes(const CV &cv, FT r_, FT ql, FT nl, FT qr, FT nr, FT vt_n, FT vt_m) {
    SedFlux<FT> f;
    f.q_rai = (r_ * qr) * vt_m;
    f.n_rai = (r_ * nr) * vt_n;
    f.q_lcl = FT(0);
    f.n_lcl = FT(0);
    if constexpr (CLOUD) {
        FT vc_n, vc_m;
        sb2006_cloud_velocity(cv, ql, r_, r_ * nl, vc_n, vc_m);
        f.q_lcl = (r_ * ql) * vc_m;
        f.n_lcl = (r_ * nl) * vc_n;
    }
    return f;
}

// flux-only evaluation of a raw point (the point after a workgroup's tile): clamps, rain PSD, fall speeds — the inline functions the
// point function itself calls, on the same operands
template <typename FT, bool LIMITED, int VEL, bool CLOUD, typename C>
__device__ __forceinline__ SedFlux<FT> sed_fluxes_of_point(const C &c, const CloudVelConsts<FT> &cv, FT rho, FT q_lcl, FT n_lcl,
                                                          FT q_rai, FT n_rai) {
    using M = Math<FT>;
    const FT eps = M::eps();
    const FT r_ = max0(rho), ql = max0(q_lcl), nl = max0(n_lcl);
    const FT qr = max0(q_rai), nr = max0(n_rai);
    const FT rs_rho = M::rsqrt(r_);
    const FT N_rai = r_ * nr;
    const FT L_rai = r_ * M::max(qr, eps);
    const SbRainPsd<FT> psd = sb2006_rain_psd<FT, LIMITED>(c, L_rai, M::max(N_rai, eps));
    FT vt_n, vt_m;
    sb2006_rain_velocity<FT, LIMITED, VEL>(c, r_, rs_rho, psd.l2_lam, N_rai < eps, qr < eps, vt_n, vt_m);
    SedFlux<FT> f = sed_fluxes<FT, CLOUD>(cv, r_, ql, nl, qr, nr, vt_n, vt_m);
    if (any_nan(rho, q_lcl, n_lcl, q_rai, n_rai)) f.q_rai = f.n_rai = f.q_lcl = f.n_lcl = M::nan();
    return f;
}

// ---- … and the same fluxes TOGETHER WITH the fall speed each one multiplies in (cmx_column_implicit_step.hip: backward-Euler sedimentation needs w itself).
// F is formed by the operations of sed_fluxes / sed_fluxes_of_point above on the same operands — (ρ⁺ χ⁺)·w — so it has their bits
// (tests/test_column_implicit_step_gpu.py compares them with inv_dz = 0); w is the value in registers, never F/(ρχ), and is not poisoned: a NaN input
// reaches the step through F.
template <typename FT> struct SedFluxW { SedFlux<FT> F, w; };

template <typename FT, bool CLOUD, typename CV>
__device__ __forceinline__ SedFluxW<FT> sed_fluxes_w(const CV &cv, FT r_, FT ql, FT nl, FT qr, FT nr, FT vt_n, FT vt_m) {
    SedFluxW<FT> o;
    o.F.q_rai = (r_ * qr) * vt_m;
    o.F.n_rai = (r_ * nr) * vt_n;
    o.w.q_rai = vt_m;
    o.w.n_rai = vt_n;
    o.F.q_lcl = o.F.n_lcl = o.w.q_lcl = o.w.n_lcl = FT(0);
    if constexpr (CLOUD) {
        FT vc_n, vc_m;
        sb2006_cloud_velocity(cv, ql, r_, r_ * nl, vc_n, vc_m);
        o.F.q_lcl = (r_ * ql) * vc_m;
        o.F.n_lcl = (r_ * nl) * vc_n;
        o.w.q_lcl = vc_m;
        o.w.n_lcl = vc_n;
    }
    return o;
}

template <typename FT, bool LIMITED, int VEL, bool CLOUD, typename C>
__device__ __forceinline__ SedFluxW<FT> sed_fluxes_w_of_point(const C &c, const CloudVelConsts<FT> &cv, FT rho, FT q_lcl, FT n_lcl, FT q_rai, FT n_rai) {
    using M = Math<FT>;
    const FT eps = M::eps();
    const FT r_ = max0(rho), ql = max0(q_lcl), nl = max0(n_lcl);
    const FT qr = max0(q_rai), nr = max0(n_rai);
    const FT rs_rho = M::rsqrt(r_);
    const FT N_rai = r_ * nr;
    const FT L_rai = r_ * M::max(qr, eps);
    const SbRainPsd<FT> psd = sb2006_rain_psd<FT, LIMITED>(c, L_rai, M::max(N_rai, eps));
    FT vt_n, vt_m;
    sb2006_rain_velocity<FT, LIMITED, VEL>(c, r_, rs_rho, psd.l2_lam, N_rai < eps, qr < eps, vt_n, vt_m);
    SedFluxW<FT> o = sed_fluxes_w<FT, CLOUD>(cv, r_, ql, nl, qr, nr, vt_n, vt_m);
    if (any_nan(rho, q_lcl, n_lcl, q_rai, n_rai)) o.F.q_rai = o.F.n_rai = o.F.q_lcl = o.F.n_lcl = M::nan();
    return o;
}

}  // namespace cmx
