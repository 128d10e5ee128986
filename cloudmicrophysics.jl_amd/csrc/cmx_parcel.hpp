// cmx_parcel.hpp — the adiabatic parcel model (the reference's parcel/ParcelModel.jl, ParcelTendencies.jl, ParcelDistributions.jl, ParcelCommon.jl), per
// parcel: the right-hand side parcel_model(dY, Y, p, t) as `parcel_rhs` and one forward-Euler step as `parcel_step`, with the host folding of the
// parameter struct.  Shared by the two kernels of cmx_parcel_kernels.hip and, under CMX_HOST_BUILD, by the g++ build of tests/native/parcel_host.cpp.
//
// Reference lines (parcel/): parcel_model ParcelModel.jl:54-187 (clip! :48-49, the state :64-76, r_act :120-123, the number sinks :142,145, the budgets
// :148-174); aerosol_activation ParcelTendencies.jl:20-41; deposition_nucleation :48-66 (MohlerAF), :92-105 (ABDINM), :107-113 (P3_dep); immersion_freezing
// :120-133 (ABIFM), :135-141 (P3_het), :156-162 (Frostenberg_mean); homogeneous_freezing :194-205 (ABHOM), :207-213 (P3_hom); condensation :220-232, :234-246;
// deposition :283-296, :298-311; distribution_moments ParcelDistributions.jl:11-23 (Monodisperse), :54-74 (Gamma); ξ, eᵥ, get_particle_activation_radius
// ParcelCommon.jl:4-33.  The options are wave-uniform branches on the flags word (include/cmx.h CMX_PARCEL_*), not template arguments: there are thousands of
// combinations and a scalar branch costs nothing against a step of several hundred instructions.
//
// Arithmetic.  Powers, roots and exponentials are evaluated in the log2 domain on the cmx_math.hpp layer like everywhere in this library; a quotient a/b is
// a·rcp(b), which keeps the IEEE special cases the reference's divisions have (x/0 = ±Inf, 0/0 = Inf/Inf = NaN, x/Inf = 0).  The order of the reference's
// expressions, its gates and its limiters are kept; min / max are Julia's (a NaN operand gives NaN: parcel_min / parcel_max), where the hardware's return
// the other operand.  A parcel with a NaN among its inputs is poisoned as a whole by the kernels (the library's NaN rule).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/cmx.h"
#include "cmx_arg.hpp"          // erfc_dev
#include "cmx_icenuc.hpp"       // saturation-pressure exponents, a_w_ice, the activity-based rate coefficients, Mohler, INP mean
#include "cmx_math.hpp"
#include "cmx_nucleation.hpp"   // P3_deposition_N_i, P3_het_N_i

namespace cmx {

template <typename FT> struct ParcelConsts {
    // thermodynamics (TDI.Rₘ, cpₘ, Lᵥ, Lₛ, Lf, air_density)
    FT R_v, R_d, Rv_over_Rd, inv_R_v, cp_d, cpm_qt, cpm_ql, cpm_qi, T_0, LH_v0, LH_s0, LH_f0, dcp_l, dcp_i, dcp_f, grav;
    // saturation pressures: the members l2_p_sat_liq_dev / a_w_ice_dev read (cmx_icenuc.hpp)
    FT aw_d0, aw_da, aw_db, inv_T_tr, ps_c0, ps_a, ps_b;
    FT inv_K, Rv_over_D, inv_eps_1m;                    // G_func_liquid / G_func_ice (Common.jl:47-102)
    FT dt, inv_dt, r_nuc, A_aer, rho_w, rho_i;
    FT four_pi, c43pi, c43pi_rho_w, c43pi_rho_i;        // 4π, 4/3 π, 4/3 π ρ
    FT gamma_lam, gamma_V;                              // Gamma distribution: λ³ = 32π N/q ρ/ρ_air; V = 4/3 π 24/λ³
    FT four_pi_rnuc2, vnuc_rho_i;                       // ABDINM surface 4π r_nuc²; 4/3 π r_nuc³ ρᵢ
    FT l2_10, l2_e;
    // AeroAct: A = A_c/T; log2 Sm = l2_smc + 1.5 log2 A; u = u_c (log2 Sm − log2 S_max)
    FT A_c, l2_Ac_Ttr, l2_smc, u_c, aero_N, half_aero_N, two_thirds;
    FT inv_tau_liq, inv_tau_ice;                        // NonEq_*_simple
    FT T_hom;                                           // P3_hom: 233.15 K (a literal in the reference)
    FT q_small;                                         // the 1e-6 of the number sinks and of r_act
    FT coef[CMX_PARCEL_NCOEF];                          // deposition_m, deposition_c, ABIFM_m, ABIFM_c, linear_c1, linear_c2 where no column overrides them
    MohlerConsts<FT> mohler;
    InpFreqConsts<FT> inp;
    P3NucConsts<FT> p3;
};

template <typename FT, typename PP> inline ParcelConsts<FT> make_parcel_consts(const PP &pp, uint32_t flags) {
    ParcelConsts<FT> c{};
    const double pi = 3.14159265358979323846, ln2 = 0.69314718055994530942;
    const auto &tp = pp.tps;
    const double Rv = tp.R_v, eps_1m = (double)Math<FT>::eps_1m();
    c.R_v = (FT)Rv; c.R_d = (FT)tp.R_d; c.Rv_over_Rd = (FT)(Rv / (double)tp.R_d); c.inv_R_v = (FT)(1.0 / Rv);
    c.cp_d = (FT)tp.cp_d; c.cpm_qt = (FT)((double)tp.cp_v - (double)tp.cp_d);
    c.cpm_ql = (FT)((double)tp.cp_l - (double)tp.cp_v); c.cpm_qi = (FT)((double)tp.cp_i - (double)tp.cp_v);
    c.T_0 = (FT)tp.T_0; c.LH_v0 = (FT)tp.LH_v0; c.LH_s0 = (FT)tp.LH_s0; c.LH_f0 = (FT)((double)tp.LH_s0 - (double)tp.LH_v0);
    c.dcp_l = (FT)((double)tp.cp_v - (double)tp.cp_l); c.dcp_i = (FT)((double)tp.cp_v - (double)tp.cp_i); c.dcp_f = (FT)((double)tp.cp_l - (double)tp.cp_i);
    c.grav = (FT)pp.grav;
    double ab[4];
    fold_saturation_exponents(tp, ab);
    c.aw_d0 = (FT)0; c.aw_da = (FT)(ab[2] - ab[0]); c.aw_db = (FT)(ab[3] - ab[1]); c.inv_T_tr = (FT)(1.0 / (double)tp.T_triple);
    c.ps_c0 = (FT)std::log2((double)tp.press_triple); c.ps_a = (FT)ab[0]; c.ps_b = (FT)ab[1];
    c.inv_K = (FT)(1.0 / std::fmax((double)pp.aps.K_therm, eps_1m));
    c.Rv_over_D = (FT)(Rv / std::fmax((double)pp.aps.D_vapor, eps_1m));
    c.inv_eps_1m = (FT)(1.0 / eps_1m);
    const double dt = pp.const_dt, r_nuc = pp.r_nuc, rho_w = pp.rho_w, rho_i = pp.rho_i;
    c.dt = (FT)dt; c.inv_dt = (FT)(1.0 / dt); c.r_nuc = (FT)r_nuc; c.A_aer = (FT)pp.A_aer; c.rho_w = (FT)rho_w; c.rho_i = (FT)rho_i;
    c.four_pi = (FT)(4.0 * pi); c.c43pi = (FT)(4.0 / 3.0 * pi); c.c43pi_rho_w = (FT)(4.0 / 3.0 * pi * rho_w); c.c43pi_rho_i = (FT)(4.0 / 3.0 * pi * rho_i);
    c.gamma_lam = (FT)(32.0 * pi); c.gamma_V = (FT)(4.0 / 3.0 * pi * 24.0);
    c.four_pi_rnuc2 = (FT)(4.0 * pi * r_nuc * r_nuc); c.vnuc_rho_i = (FT)(4.0 / 3.0 * pi * r_nuc * r_nuc * r_nuc * rho_i);
    c.l2_10 = (FT)kLog2_10; c.l2_e = (FT)kIceNucLog2e;
    const auto &ap = pp.aap;
    const double A_c = 2.0 * (double)ap.sigma * (double)ap.M_w / (double)ap.rho_w / (double)ap.R;
    c.A_c = (FT)A_c; c.l2_Ac_Ttr = (FT)std::log2(A_c / (double)tp.T_triple);
    c.l2_smc = (FT)(std::log2(2.0 / std::sqrt((double)pp.aero_kappa)) - 1.5 * std::log2(3.0 * r_nuc));
    c.u_c = (FT)(2.0 * ln2 / (3.0 * std::sqrt(2.0) * std::log((double)pp.aero_sigma_g)));
    c.aero_N = (FT)pp.aero_N; c.half_aero_N = (FT)(0.5 * (double)pp.aero_N); c.two_thirds = (FT)(2.0 / 3.0);
    c.inv_tau_liq = (FT)(1.0 / (double)pp.tau_relax_liq); c.inv_tau_ice = (FT)(1.0 / (double)pp.tau_relax_ice);
    c.T_hom = (FT)233.15; c.q_small = (FT)1e-6;
    // a coefficient pair whose scheme is off is never read: zero, so that a stray value in the struct cannot poison the parcel (NaN rule)
    const bool abdinm = (flags & CMX_PARCEL_DEP_MASK) == CMX_PARCEL_DEP_ABDINM, abifm = (flags & CMX_PARCEL_HET_MASK) == CMX_PARCEL_HET_ABIFM,
               abhom = (flags & CMX_PARCEL_HOM_MASK) == CMX_PARCEL_HOM_ABHOM;
    c.coef[CMX_PARCEL_COEF_DEPOSITION_M] = abdinm ? (FT)pp.aerosol_deposition.deposition_m : FT(0);
    c.coef[CMX_PARCEL_COEF_DEPOSITION_C] = abdinm ? (FT)pp.aerosol_deposition.deposition_c : FT(0);
    c.coef[CMX_PARCEL_COEF_ABIFM_M] = abifm ? (FT)pp.aerosol_abifm.ABIFM_m : FT(0);
    c.coef[CMX_PARCEL_COEF_ABIFM_C] = abifm ? (FT)pp.aerosol_abifm.ABIFM_c : FT(0);
    c.coef[CMX_PARCEL_COEF_LINEAR_C1] = abhom ? (FT)pp.homogeneous.linear_c1 : FT(0);
    c.coef[CMX_PARCEL_COEF_LINEAR_C2] = abhom ? (FT)pp.homogeneous.linear_c2 : FT(0);
    c.mohler = make_mohler_consts<FT>(pp.aerosol_mohler, pp.deposition);
    c.inp = make_inp_consts<FT>(pp.ip);
    c.p3 = make_p3_nucleation_consts<FT>(pp.p3);
    return c;
}

// CMX_OK, or why a flags word cannot run: a value the reference has but this library does not build is CMX_ERR_UNSUPPORTED, anything else CMX_ERR_BAD_ARG
inline int32_t parcel_flags_status(uint32_t fl) {
    constexpr uint32_t known = CMX_PARCEL_AERO_ACT | CMX_PARCEL_DEP_MASK | CMX_PARCEL_HET_MASK | CMX_PARCEL_HOM_MASK | CMX_PARCEL_COND_MASK |
                               CMX_PARCEL_DEPGROWTH_MASK | CMX_PARCEL_LIQ_MASK | CMX_PARCEL_ICE_GAMMA | CMX_PARCEL_PRESCRIBED_THERMODYNAMICS;
    if (fl & ~known) return CMX_ERR_BAD_ARG;
    const uint32_t dep = fl & CMX_PARCEL_DEP_MASK, het = fl & CMX_PARCEL_HET_MASK, hom = fl & CMX_PARCEL_HOM_MASK, ce = fl & CMX_PARCEL_COND_MASK,
                   ds = fl & CMX_PARCEL_DEPGROWTH_MASK, liq = fl & CMX_PARCEL_LIQ_MASK;
    if (dep > CMX_PARCEL_DEP_P3 || het > CMX_PARCEL_HET_FROSTENBERG_STOCHASTIC || hom > CMX_PARCEL_HOM_P3 || liq > CMX_PARCEL_LIQ_MONODISPERSE_MIX)
        return CMX_ERR_BAD_ARG;
    if (dep == CMX_PARCEL_DEP_MOHLER_RATE || het == CMX_PARCEL_HET_FROSTENBERG_RANDOM || het == CMX_PARCEL_HET_FROSTENBERG_STOCHASTIC ||
        ce == CMX_PARCEL_COND_NONEQ || ds == CMX_PARCEL_DEPGROWTH_NONEQ || liq == CMX_PARCEL_LIQ_MONODISPERSE_MIX ||
        (fl & CMX_PARCEL_PRESCRIBED_THERMODYNAMICS))
        return CMX_ERR_UNSUPPORTED;
    return CMX_OK;
}

// Julia's min / max / clip!: a NaN operand gives NaN
template <typename FT> __device__ __forceinline__ FT parcel_min(FT a, FT b) {
    const FT m = Math<FT>::min(a, b);
    return any_nan(a, b) ? Math<FT>::nan() : m;
}
template <typename FT> __device__ __forceinline__ FT parcel_max(FT a, FT b) {
    const FT m = Math<FT>::max(a, b);
    return any_nan(a, b) ? Math<FT>::nan() : m;
}
template <typename FT> __device__ __forceinline__ FT parcel_abs(FT x) {
    if constexpr (sizeof(FT) == 8) return __builtin_fabs(x);
    else return __builtin_fabsf(x);
}
// Subnormal operands.  A number concentration that freezing depletes by a fixed share per step (dN = −J A N) decays geometrically through the subnormal
// range of Float32 before it reaches zero, and so does a content that evaporates.  The kernels run with subnormals on: compares, adds and multiplies keep
// them, as the reference's arithmetic does, but v_rcp_f32 and v_log_f32 read a subnormal operand as zero, so q·rcp(N) would be Inf where q/N is an ordinary
// number and the parcel would end as Inf·0.  The quotients by a state value and the cube root therefore scale such an operand into the normal range by a power
// of two (exact) and scale the result back; an operand in the normal range takes factors of one and keeps its bits.  Float64: v_rcp_f64 and the table
// functions handle subnormals themselves.
template <typename FT> __device__ __forceinline__ FT parcel_quot(FT a, FT b) {
    if constexpr (sizeof(FT) == 8) {
        return Math<FT>::div(a, b);
    } else {
        const FT s = parcel_abs<FT>(b) < FT(0x1p-100f) ? FT(0x1p64f) : FT(1);      // a NaN compares false: factor one, NaN out
        return (a * Math<FT>::rcp(b * s)) * s;
    }
}
template <typename FT> __device__ __forceinline__ FT parcel_cbrt(FT x) {
    if constexpr (sizeof(FT) == 8) {
        return Math<FT>::exp2(Math<FT>::log2(x) * FT(1.0 / 3.0));
    } else {
        const bool tiny = x < FT(0x1p-96f);
        const FT r = Math<FT>::exp2(Math<FT>::log2(tiny ? x * FT(0x1p96f) : x) * FT(1.0 / 3.0));
        return tiny ? r * FT(0x1p-32f) : r;
    }
}

// distribution_moments: mean radius r and mean volume V of a Monodisperse or Gamma population of N particles per kg holding q (ParcelDistributions.jl)
template <typename FT, typename C>
__device__ __forceinline__ void parcel_moments(const C &c, bool gamma, FT q, FT N, FT rho, FT c43pi, FT rho_air, FT inv_rho_air, FT &r, FT &V) {
    using M = Math<FT>;
    if (gamma) {                                                      // wave-uniform
        const FT lam = parcel_cbrt<FT>(parcel_quot<FT>(c.gamma_lam * N, q) * rho * inv_rho_air);      // cbrt(32 π N / q ρ / ρ_air)
        const FT inv_lam = M::rcp(lam);
        r = FT(2) * inv_lam;
        V = c.gamma_V * (inv_lam * inv_lam * inv_lam);
    } else {
        r = parcel_cbrt<FT>(M::div(M::div(parcel_quot<FT>(q, N), c43pi), rho) * rho_air);            // cbrt(q / N / (4/3 π) / ρ ρ_air)
        V = c43pi * (r * r * r);
    }
    const bool none = m_or(N == FT(0), q == FT(0));
    r = none ? FT(0) : r;
    V = none ? FT(0) : V;
}

// the ifelse of condensation / deposition: growth limited by the vapour, loss by the condensate, per step
template <typename FT> __device__ __forceinline__ FT parcel_limit(FT dq, FT q_vap_per_dt, FT q_cond_per_dt) {
    const FT up = parcel_min<FT>(dq, q_vap_per_dt), down = -parcel_min<FT>(parcel_abs<FT>(dq), q_cond_per_dt);
    return dq > FT(0) ? up : down;
}

// k: the six activity-based coefficients of THIS parcel (cmx_parcel_coefficient_column).  dY: rows 1–9 of the reference's dY.  proc: cmx_parcel_process_column.
template <typename FT, typename C>
__device__ __forceinline__ void parcel_rhs(const C &c, const uint32_t fl, const FT (&Y)[CMX_PARCEL_NSTATE], const FT w, const FT (&k)[CMX_PARCEL_NCOEF],
                                           FT (&dY)[CMX_PARCEL_NSTATE], FT (&proc)[CMX_PARCEL_NPROC]) {
    using M = Math<FT>;
    const FT eps = FT(M::eps()), zero = FT(0);
    const uint32_t dep = fl & CMX_PARCEL_DEP_MASK, het = fl & CMX_PARCEL_HET_MASK, hom = fl & CMX_PARCEL_HOM_MASK, ce = fl & CMX_PARCEL_COND_MASK,
                   ds = fl & CMX_PARCEL_DEPGROWTH_MASK;
    // state: the clip of rows 4–9 only                                                                          ParcelModel.jl:64-76
    const FT S = Y[0], p = Y[1], T = Y[2];
    const FT qv = parcel_max<FT>(Y[3], zero), ql = parcel_max<FT>(Y[4], zero), qi = parcel_max<FT>(Y[5], zero);
    const FT Na = parcel_max<FT>(Y[6], zero), Nl = parcel_max<FT>(Y[7], zero), Ni = parcel_max<FT>(Y[8], zero);
    const FT qt = qv + ql + qi;
    // moist-air constants                                                                                       :89-94
    const FT R_air = c.R_d * (FT(1) + (c.Rv_over_Rd - FT(1)) * qt - c.Rv_over_Rd * (ql + qi));
    const FT cp_air = M::fma(c.cpm_qi, qi, M::fma(c.cpm_ql, ql, M::fma(c.cpm_qt, qt, c.cp_d)));
    const FT dT0 = T - c.T_0;
    const FT L_vap = M::fma(c.dcp_l, dT0, c.LH_v0), L_subl = M::fma(c.dcp_i, dT0, c.LH_s0), L_fus = M::fma(c.dcp_f, dT0, c.LH_f0);
    const FT inv_T = M::rcp(T), inv_R = M::rcp(R_air), inv_cp = M::rcp(cp_air);
    const FT rho_air = p * inv_R * inv_T;
    const FT inv_rho = M::rcp(rho_air);
    // vapour pressures                                                                                          :97-98
    const FT e = qv * p * c.R_v * inv_R;
    const FT esl = M::exp2(l2_p_sat_liq_dev<FT>(c, T, inv_T));
    const FT inv_esl = M::rcp(esl);
    // over ice: a_w_ice = e_si/e_sl, ξ = e_sl/e_si (ParcelCommon.jl:4-6) — only the options that read them
    const bool need_ice = dep == CMX_PARCEL_DEP_MOHLER_AF || dep == CMX_PARCEL_DEP_ABDINM || het == CMX_PARCEL_HET_ABIFM || hom == CMX_PARCEL_HOM_ABHOM ||
                          ds != 0;
    FT a_w_ice = zero, xi = zero;
    if (need_ice) {
        a_w_ice = a_w_ice_dev<FT>(c, T, inv_T);
        xi = M::rcp(a_w_ice);
    }
    // size distributions                                                                                        :114-116
    FT r_l, V_l, r_i = zero, V_i = zero;
    parcel_moments<FT>(c, (fl & CMX_PARCEL_LIQ_MASK) == CMX_PARCEL_LIQ_GAMMA, ql, Nl, c.rho_w, c.c43pi, rho_air, inv_rho, r_l, V_l);
    if (ds == CMX_PARCEL_DEPGROWTH_DEPOSITION) parcel_moments<FT>(c, (fl & CMX_PARCEL_ICE_GAMMA) != 0, qi, Ni, c.rho_i, c.c43pi, rho_air, inv_rho, r_i, V_i);

    // aerosol activation                                                                                        :119-124, ParcelTendencies.jl:20-41
    FT dNl_act = zero;
    const FT sm1 = S - FT(1);
    if (fl & CMX_PARCEL_AERO_ACT) {
        const FT smax = parcel_max<FT>(zero, sm1);
        const FT l2_A = c.l2_Ac_Ttr - M::log2(T * c.inv_T_tr);                                 // A = 2σ M_w/(ρ_w R T)
        const FT u = c.u_c * (M::fma(FT(1.5), l2_A, c.l2_smc) - M::log2(smax));              // 2 log(Sm/S_max)/3/√2/log σ_g
        dNl_act = parcel_max<FT>(zero, c.half_aero_N * erfc_dev<FT>(u) - (c.aero_N - Na));    // N ½ (1 − erf u) − (Nₐ⁰ − Nₐ)
    }
    const FT r_crit = parcel_min<FT>(c.q_small, M::div(c.two_thirds * (c.A_c * inv_T), sm1));   // get_particle_activation_radius
    const FT r_act = m_or(dNl_act < eps, sm1 < eps) ? c.r_nuc : r_crit;
    const FT dql_act = dNl_act * (c.c43pi_rho_w * (r_act * r_act * r_act)) * inv_rho;

    // Δa_w of the activity-based schemes from the vapour pressure (ABDINM, ABIFM): a_w_eT(e, T) − a_w_ice(T)
    const FT d_aw_e = e * inv_esl - a_w_ice;
    // deposition nucleation                                                                                     :128-129
    FT dNi_dep = zero;
    if (dep == CMX_PARCEL_DEP_MOHLER_AF) {
        const FT Si = xi * S;
        const FT AF = Si >= c.mohler.S_i_max ? zero : mohler_activated_fraction_dev<FT>(c.mohler, Si, T > c.mohler.T_thr);   // Sᵢ ≥ Sᵢ_max: no dust is activated
        dNi_dep = parcel_max<FT>(zero, AF * Na - Ni) * c.inv_dt;
    } else if (dep == CMX_PARCEL_DEP_ABDINM) {
        const FT J = activity_J_dev<FT>(k[CMX_PARCEL_COEF_DEPOSITION_M] * c.l2_10, (k[CMX_PARCEL_COEF_DEPOSITION_C] + FT(4)) * c.l2_10, d_aw_e);
        dNi_dep = parcel_min<FT>(J * Na * c.four_pi_rnuc2, Na * c.inv_dt);
    } else if (dep == CMX_PARCEL_DEP_P3) {
        const FT N_dep = p3_deposition_N_i<FT>(c.p3, T);
        dNi_dep = parcel_min<FT>(parcel_max<FT>(zero, (N_dep - Ni) * c.inv_dt), Na * c.inv_dt);
    }
    const FT dqi_dep = dNi_dep * c.vnuc_rho_i * inv_rho;

    // heterogeneous (immersion) freezing                                                                        :132-134
    FT dNi_imm = zero;
    if (het == CMX_PARCEL_HET_ABIFM) {
        const FT J = activity_J_dev<FT>(k[CMX_PARCEL_COEF_ABIFM_M] * c.l2_10, (k[CMX_PARCEL_COEF_ABIFM_C] + FT(4)) * c.l2_10, d_aw_e);
        dNi_imm = parcel_min<FT>(J * Nl * c.A_aer, Nl * c.inv_dt);
    } else if (het == CMX_PARCEL_HET_P3) {
        const FT N_het = p3_het_N_i<FT>(c.p3, T, Nl, V_l, c.dt);
        dNi_imm = parcel_min<FT>(parcel_max<FT>(zero, (N_het - Ni) * c.inv_dt), Nl * c.inv_dt);
    } else if (het == CMX_PARCEL_HET_FROSTENBERG_MEAN) {
        const FT INPC = M::exp2(inp_concentration_mean_dev<FT>(c.inp, T) * c.l2_e);
        dNi_imm = parcel_min<FT>(Nl, parcel_max<FT>(zero, INPC - Ni)) * c.inv_dt;
    }
    const FT dqi_imm = dNi_imm * V_l * c.rho_i * inv_rho;

    // homogeneous freezing                                                                                      :137-138
    FT dNi_hom = zero;
    if (hom == CMX_PARCEL_HOM_ABHOM) {
        const FT d_aw_S = (esl * S) * inv_esl - a_w_ice;                                        // e = e_sl·Sₗ, ParcelTendencies.jl:199
        const FT J = activity_J_dev<FT>(k[CMX_PARCEL_COEF_LINEAR_C2] * c.l2_10, (k[CMX_PARCEL_COEF_LINEAR_C1] + FT(6)) * c.l2_10, d_aw_S);
        dNi_hom = parcel_min<FT>(J * Nl * V_l, Nl * c.inv_dt);
    } else if (hom == CMX_PARCEL_HOM_P3) {
        dNi_hom = m_and(T < c.T_hom, Nl > zero) ? Nl * c.inv_dt : zero;
    }
    const FT dqi_hom = dNi_hom * V_l * c.rho_i * inv_rho;

    // condensation / evaporation                                                                                :141-142
    FT dql_ce = zero;
    const FT LoT_v = L_vap * inv_T;
    if (ce == CMX_PARCEL_COND_CONDENSATION) {
        const FT G_l = M::rcp(M::fma(LoT_v * c.inv_K, LoT_v * c.inv_R_v - FT(1), c.Rv_over_D * T * M::min(inv_esl, c.inv_eps_1m)));   // G_func_liquid
        const FT dq = c.four_pi * inv_rho * sm1 * G_l * r_l * Nl;
        dql_ce = parcel_limit<FT>(dq, qv * c.inv_dt, ql * c.inv_dt);
    } else if (ce == CMX_PARCEL_COND_NONEQ_SIMPLE) {
        dql_ce = (parcel_max<FT>(S * qv - qv, zero) - ql) * c.inv_tau_liq;
    }
    const FT dNl_ce = m_and(dql_ce < zero, ql > zero, ql < c.q_small) ? parcel_quot<FT>(Nl * dql_ce, ql) : zero;
    // deposition / sublimation                                                                                  :144-145
    FT dqi_ds = zero;
    if (ds == CMX_PARCEL_DEPGROWTH_DEPOSITION) {
        const FT Si = xi * S, LoT_s = L_subl * inv_T;
        const FT inv_esi = xi * inv_esl;                                                        // 1/e_si = ξ/e_sl
        const FT G_i = M::rcp(M::fma(LoT_s * c.inv_K, LoT_s * c.inv_R_v - FT(1), c.Rv_over_D * T * M::min(inv_esi, c.inv_eps_1m)));   // G_func_ice
        const FT dq = c.four_pi * inv_rho * (Si - FT(1)) * G_i * r_i * Ni;
        dqi_ds = parcel_limit<FT>(dq, qv * c.inv_dt, qi * c.inv_dt);
    } else if (ds == CMX_PARCEL_DEPGROWTH_NONEQ_SIMPLE) {
        const FT Si = xi * S;
        dqi_ds = (parcel_max<FT>(Si * qv - qv, zero) - qi) * c.inv_tau_ice;
    }
    const FT dNi_ds = m_and(dqi_ds < zero, qi > zero, qi < c.q_small) ? parcel_quot<FT>(Ni * dqi_ds, qi) : zero;

    // number and water budgets                                                                                  :148-159
    const FT dNi = dNi_dep + dNi_imm + dNi_hom + dNi_ds;
    const FT dNa = -dNi_dep - dNl_act;
    const FT dNl = dNl_act - dNi_imm - dNi_hom + dNl_ce;
    const FT dql_v2l = dql_ce + dql_act, dqi_l2i = dqi_imm + dqi_hom, dqi_v2i = dqi_dep + dqi_ds;
    const FT dqi = dqi_v2i + dqi_l2i, dql = dql_v2l - dqi_l2i, dqv = -dql_v2l - dqi_v2i;
    // pressure, temperature, saturation ratio                                                                  :161-174
    const FT dp = -p * c.grav * inv_R * inv_T * w;
    const FT dT = -c.grav * inv_cp * w + L_vap * inv_cp * dql_v2l + L_fus * inv_cp * dqi_l2i + L_subl * inv_cp * dqi_v2i;
    const FT de = dqv * p * c.R_v * inv_R + qv * dp * c.R_v * inv_R;
    const FT desl = L_vap * esl * c.inv_R_v * (inv_T * inv_T) * dT;
    const FT dS = inv_esl * de - e * (inv_esl * inv_esl) * desl;

    dY[0] = dS; dY[1] = dp; dY[2] = dT; dY[3] = dqv; dY[4] = dql; dY[5] = dqi; dY[6] = dNa; dY[7] = dNl; dY[8] = dNi;
    proc[CMX_PARCEL_PROC_DN_LIQ_ACT] = dNl_act; proc[CMX_PARCEL_PROC_DN_ICE_DEP] = dNi_dep; proc[CMX_PARCEL_PROC_DN_ICE_IMM] = dNi_imm;
    proc[CMX_PARCEL_PROC_DN_ICE_HOM] = dNi_hom; proc[CMX_PARCEL_PROC_DQ_LIQ_CE] = dql_ce; proc[CMX_PARCEL_PROC_DQ_ICE_DS] = dqi_ds;
}

// one step of ODE.Euler with dt = const_dt: Y ← Y + const_dt·dY on the UNCLIPPED rows (the clip is part of the right-hand side only)
template <typename FT, typename C>
__device__ __forceinline__ void parcel_step(const C &c, const uint32_t fl, FT (&Y)[CMX_PARCEL_NSTATE], const FT w, const FT (&k)[CMX_PARCEL_NCOEF]) {
    FT dY[CMX_PARCEL_NSTATE], proc[CMX_PARCEL_NPROC];
    parcel_rhs<FT>(c, fl, Y, w, k, dY, proc);
#pragma unroll
    for (int j = 0; j < CMX_PARCEL_NSTATE; ++j) Y[j] = Y[j] + c.dt * dY[j];
}

// the library's NaN rule for a parcel: a NaN among the nine state values, w or the six coefficients
template <typename FT> __device__ __forceinline__ bool parcel_inputs_nan(const FT (&Y)[CMX_PARCEL_NSTATE], const FT w, const FT (&k)[CMX_PARCEL_NCOEF]) {
    return any_nan(Y[0], Y[1], Y[2], Y[3], Y[4], Y[5], Y[6], Y[7], Y[8], w, k[0], k[1], k[2], k[3], k[4], k[5]);
}

}  // namespace cmx
