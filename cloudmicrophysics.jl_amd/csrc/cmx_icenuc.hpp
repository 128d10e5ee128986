// cmx_icenuc.hpp — host-folded constants and per-point functions of the ice-nucleation subsystem: water activity (a_w_ice, a_w_eT, the H2SO4 solution),
// the activity-based rate coefficients (ABIFM, deposition_J, the Koop linear fit), the Mohler-2006 activated fraction and the Frostenberg-2023 INP
// mean.  Shared by the streaming kernels of cmx_icenuc_kernels.hip and by the parcel model (cmx_parcel.hpp); compilable under CMX_HOST_BUILD.
// The functions take any constants struct that has the members they read (IceNucConsts here, ParcelConsts in cmx_parcel.hpp).
//
// Reference (src = the reference's src/): CO.a_w_ice / a_w_eT  Common.jl:250-271; CMI_het.ABIFM_J IceNucleation.jl:124-134; deposition_J :81-102;
// dust_activated_number_fraction :44-53; INP_concentration_mean :250-253; CMI_hom.homogeneous_J_linear :581-584.
#pragma once
#include <cmath>

#include "cmx_math.hpp"

namespace cmx {

constexpr double kLog2_10 = 3.3219280948873623479, kIceNucLog2e = 1.4426950408889634074;

template <typename FT> struct IceNucConsts {
    // log2 a_w_ice(T) = d0 + da·log2(T/T_tr) + db·(1/T_tr − 1/T)
    FT aw_d0, aw_da, aw_db, inv_T_tr;
    // log2 p_sat,liq(T) = c0 + a·log2(T/T_tr) + b·(1/T_tr − 1/T)   (a_w_eT)
    FT ps_c0, ps_a, ps_b;
    FT abifm_m_l2, abifm_c_l2;        // (m Δ + c + 4)·log2(10)
    double c1, c2, c3, c4;            // Koop cubic, evaluated in double
    FT lin_c1_l2, lin_c2_l2;          // (linear_c2 Δ + linear_c1 + 6)·log2(10)
    FT d_min, d_max;
    FT l2_four_pi, l2_four_thirds_pi;
    // H2SO4 solution (Common.jl:188-220): log2 p_sol[Pa] = hp1(x) + hp2(x)/T,  hp1 = Σ hp1[m] x^m (m ≤ 3), hp2 = Σ hp2[m] x^m (m ≤ 2)
    FT hp1[4], hp2[3];
};

template <typename FT, typename HS> static void add_h2so4_consts(IceNucConsts<FT> &c, const HS &h) {
    const double l2e = 1.4426950408889634074, w2 = h.w_2;
    c.hp1[0] = (FT)((double)h.c1 * l2e + std::log2(100.0));   // ·100: mbar → Pa
    c.hp1[1] = (FT)(-(double)h.c2 * l2e);
    c.hp1[2] = (FT)((double)h.c3 * w2 * l2e);                  // c3 x w_h, w_h = w_2 x
    c.hp1[3] = (FT)(-(double)h.c4 * w2 * w2 * l2e);            // −c4 x w_h²
    c.hp2[0] = (FT)((double)h.c5 * l2e);
    c.hp2[1] = (FT)((double)h.c6 * l2e);
    c.hp2[2] = (FT)(-(double)h.c7 * w2 * l2e);                 // −c7 x w_h
}
// log2 of CO.H2SO4_soln_saturation_vapor_pressure(prs, x, T) [Pa]
template <typename FT, typename C> __device__ __forceinline__ FT l2_p_sol_dev(const C &c, FT x, FT inv_T) {
    using M = Math<FT>;
    const FT p1 = M::fma(M::fma(M::fma(c.hp1[3], x, c.hp1[2]), x, c.hp1[1]), x, c.hp1[0]);
    const FT p2 = M::fma(M::fma(c.hp2[2], x, c.hp2[1]), x, c.hp2[0]);
    return M::fma(p2, inv_T, p1);
}
template <typename FT, typename C> __device__ __forceinline__ FT l2_p_sat_liq_dev(const C &c, FT T, FT inv_T) {
    using M = Math<FT>;
    return M::fma(c.ps_a, M::log2(T * c.inv_T_tr), M::fma(c.ps_b, c.inv_T_tr - inv_T, c.ps_c0));
}

// The Rankine–Kirchhoff exponents of the two saturation pressures, log2 p_sat(T) = c0 + a·log2(T/T_tr) + b·(1/T_tr − 1/T), folded in double:
// out[0..1] = a, b over liquid, out[2..3] = a, b over ice
template <typename TH> inline void fold_saturation_exponents(const TH &tp, double (&out)[4]) {
    const double l2e = 1.4426950408889634074;
    const double Rv = tp.R_v, T0 = tp.T_0;
    const double dcp_l = (double)tp.cp_v - (double)tp.cp_l, dcp_i = (double)tp.cp_v - (double)tp.cp_i;
    out[0] = dcp_l / Rv; out[2] = dcp_i / Rv;
    out[1] = ((double)tp.LH_v0 - dcp_l * T0) / Rv * l2e; out[3] = ((double)tp.LH_s0 - dcp_i * T0) / Rv * l2e;
}

template <typename FT, typename TH, typename DU, typename KO>
static IceNucConsts<FT> make_icenuc_consts(const TH &tp, const DU *dust, const KO *koop) {
    IceNucConsts<FT> c{};
    const double l2_10 = 3.3219280948873623479, pi = 3.14159265358979323846;
    const double Ttr = tp.T_triple;
    double ab[4];
    fold_saturation_exponents(tp, ab);
    const double a_l = ab[0], b_l = ab[1], a_i = ab[2], b_i = ab[3];
    c.aw_d0 = (FT)0;                                   // same triple-point pressure for both phases
    c.aw_da = (FT)(a_i - a_l);
    c.aw_db = (FT)(b_i - b_l);
    c.inv_T_tr = (FT)(1.0 / Ttr);
    c.ps_c0 = (FT)std::log2((double)tp.press_triple);
    c.ps_a = (FT)a_l;
    c.ps_b = (FT)b_l;
    if (dust) {
        c.abifm_m_l2 = (FT)((double)dust->ABIFM_m * l2_10);
        c.abifm_c_l2 = (FT)(((double)dust->ABIFM_c + 4.0) * l2_10);
    }
    if (koop) {
        c.c1 = koop->c1; c.c2 = koop->c2; c.c3 = koop->c3; c.c4 = koop->c4;
        c.lin_c1_l2 = (FT)(((double)koop->linear_c1 + 6.0) * l2_10);
        c.lin_c2_l2 = (FT)((double)koop->linear_c2 * l2_10);
        c.d_min = (FT)koop->delta_a_w_min;
        c.d_max = (FT)koop->delta_a_w_max;
    }
    c.l2_four_pi = (FT)std::log2(4.0 * pi);
    c.l2_four_thirds_pi = (FT)std::log2(4.0 / 3.0 * pi);
    return c;
}

template <typename FT, typename C> __device__ __forceinline__ FT a_w_ice_dev(const C &c, FT T, FT inv_T) {
    using M = Math<FT>;
    return M::exp2(M::fma(c.aw_da, M::log2(T * c.inv_T_tr), M::fma(c.aw_db, c.inv_T_tr - inv_T, c.aw_d0)));
}

// An activity-based rate coefficient 10^(m Δa_w + c + shift) as one exponential of the log2-domain line (m_l2 = m log2 10, c_l2 = (c + shift) log2 10):
// ABIFM_J and deposition_J (shift 4: cm⁻² → m⁻²), homogeneous_J_linear (shift 6: cm⁻³ → m⁻³)
template <typename FT> __device__ __forceinline__ FT l2_activity_J_dev(FT m_l2, FT c_l2, FT delta_a_w) { return Math<FT>::fma(m_l2, delta_a_w, c_l2); }
template <typename FT> __device__ __forceinline__ FT activity_J_dev(FT m_l2, FT c_l2, FT delta_a_w) {
    return Math<FT>::exp2(l2_activity_J_dev<FT>(m_l2, c_l2, delta_a_w));
}

// CMI_het.dust_activated_number_fraction without its assertion (the callers decide what S_i ≥ S_i_max means): max(0, exp(a (S_i − S₀)) − 1)
template <typename FT> struct MohlerConsts { FT S_i_max, T_thr, S0_warm, S0_cold, a_warm_l2e, a_cold_l2e, a_warm, a_cold; };
template <typename FT, typename DU, typename IP> inline MohlerConsts<FT> make_mohler_consts(const DU &dust, const IP &ip) {
    const double l2e = 1.4426950408889634074;
    return MohlerConsts<FT>{(FT)ip.S_i_max, (FT)ip.T_thr, (FT)dust.S0_warm, (FT)dust.S0_cold, (FT)((double)dust.a_warm * l2e),
                            (FT)((double)dust.a_cold * l2e), (FT)dust.a_warm, (FT)dust.a_cold};
}
template <typename FT, typename C> __device__ __forceinline__ FT mohler_activated_fraction_dev(const C &c, FT Si, bool warm) {
    using M = Math<FT>;
    return M::max(FT(0), M::exp2((warm ? c.a_warm_l2e : c.a_cold_l2e) * (Si - (warm ? c.S0_warm : c.S0_cold))) - FT(1));
}

// CMI_het.INP_concentration_mean: μ(T) = 9 log(−b T_c/10) − log a, T_c = min(T − T_freeze, 0)
template <typename FT> struct InpFreqConsts { FT T_freeze, b10, log_a, ln2, inv_2s2_l2e, inv_norm; };
template <typename FT, typename IP> inline InpFreqConsts<FT> make_inp_consts(const IP &ip) {
    const double l2e = 1.4426950408889634074, pi = 3.14159265358979323846, two_s2 = 2.0 * (double)ip.sigma * (double)ip.sigma;
    return InpFreqConsts<FT>{(FT)ip.T_freeze, (FT)((double)ip.b / 10.0), (FT)ip.log_a, (FT)0.69314718055994530942, (FT)(l2e / two_s2),
                             (FT)(1.0 / std::sqrt(pi * two_s2))};
}
template <typename FT, typename C> __device__ __forceinline__ FT inp_concentration_mean_dev(const C &c, FT T) {
    using M = Math<FT>;
    const FT Tc = M::min(T - c.T_freeze, FT(0));
    return M::fma(FT(9) * c.ln2, M::log2(-(c.b10 * Tc)), -c.log_a);          // 9 log(−b T_c/10) − log a
}

}  // namespace cmx
