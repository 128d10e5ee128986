// cmx_mp1m_vel.hpp — bulk fall speeds of the 1-moment species, per point: Blk1M rain / snow (CM1.terminal_velocity,
// /root/reference/src/Microphysics1M.jl:223-249), Chen-2022 rain and snow mass-weighted over the Marshall–Palmer PSD (CM1:251-297,
// Common.jl:290-350,414-422), cloud liquid in the Stokes regime and cloud ice by Chen-2022 small ice at the mean-volume diameter
// (CMNonEq.terminal_velocity, MicrophysicsNonEq.jl:250-281).  Shared by the velocity / sedimentation kernels (cmx_mp1m_kernels.hip)
// and the fused 1-moment column step (cmx_mp1m_column.hip).
#pragma once
#include <type_traits>
#include <utility>

#include "cmx_mp1m.hpp"

namespace cmx {

template <typename FT> struct Vel1mConsts {
    FT eps_1m, l2_eps, lam_a_rai, lam_b_rai, lam_floor_rai, lam_a_sno, lam_b_sno, lam_floor_sno, sno_l2_mu, sno_nu;
    FT rho_w, vt_k_rai, vt_e_rai, vt_k_sno, vt_e_sno;
    FT ch_rho0_l2e, ch_a[3], ch_a3_pow, ch_b[3], ch_b_rho, ch_c1000[3], l2_1000;
    ChenGamma<FT> chg;   // Γ(b_i(ρ) + 4)/3! as polynomials in ρ (cmx_math.hpp)
    // cloud liquid, Stokes (NonEq:250-265): v = st_pref (ρw/ρ − 1) D², D³ = st_D3 ρ q
    FT st_pref, st_rho_w, st_D3;
    // cloud ice, Chen-2022 small ice reduced at ρᵢ(cloud ice) (NonEq:267-281, Common.jl:304-325): D³ = ci_D3 ρ q
    FT ci_D3, ci_A, ci_B, ci_C, ci_E, ci_F, ci_c2;
    // snow, Chen-2022 large ice reduced at ρᵢ(snow), mass-weighted over the Marshall–Palmer PSD (CM1:272-297):
    // ϕ^κ Γ(b+4)/3! folded into the amplitudes
    FT sn_A, sn_a1, sn_b1, sn_a2, sn_H, sn_b2, sn_c2;
};
// … and the snow fall speed of a given shape (CM1:299-324, vel_snow_chen<FT, true>): one constant more, the power of λ_D⁻¹ in term 2.  It follows
// every member of Vel1mConsts at the member's own offset; a derived struct instead of a longer Vel1mConsts keeps the kernel-argument
// segments of the kernels without a shape byte for byte (a longer struct would move the by-value arguments after it).
template <typename FT> struct Vel1mShapeConsts : Vel1mConsts<FT> {
    FT sn_e2;   // κα − 4 (−4 for the fixed aspect ratio)
};

// (VC below: Vel1mConsts<FT>, possibly in the constant address space — kernels whose constants overflow the SGPR file read them through the
// kernel-argument pointer, cmx_math.hpp front_consts)
// log2 λ⁻¹ of rain / snow (CM1.lambda_inverse :126-152, get_n0 :83-86) from ρ⁺ = max(0, ρ) and q
template <typename FT, typename VC> __device__ __forceinline__ FT vel_l2_li_rain(const VC &c, FT rp, FT q) {
    using M = Math<FT>;
    return M::max(c.lam_floor_rai, M::fma(log2_floored(rp * M::max(FT(0), q)), c.lam_a_rai, c.lam_b_rai));
}
template <typename FT, typename VC> __device__ __forceinline__ FT vel_l2_li_snow(const VC &c, FT rp, FT q) {
    using M = Math<FT>;
    const FT l2_rq = log2_floored(rp * M::max(FT(0), q));
    const FT l2_n0 = q > c.eps_1m ? FT(M::fma(c.sno_nu, l2_rq, c.sno_l2_mu)) : FT(c.l2_eps);
    return M::max(c.lam_floor_sno, M::fma(l2_rq - M::max(l2_n0, c.l2_eps), c.lam_a_sno, c.lam_b_sno));
}
// CM1.terminal_velocity(::Rain / ::Snow, ::Blk1MVelType, ρ, q) — CM1:223-249
template <typename FT, typename VC> __device__ __forceinline__ FT vel_rain_blk1m(const VC &c, FT rho, FT l2_li, FT q) {
    using M = Math<FT>;
    const FT sq = M::sqrt(M::max(c.rho_w * M::rcp(rho) - FT(1), FT(0)));
    return q > c.eps_1m ? FT((c.vt_k_rai * sq) * M::exp2_fin(c.vt_e_rai * l2_li)) : FT(0);      // l2_li: floored, finite
}
template <typename FT, typename VC> __device__ __forceinline__ FT vel_snow_blk1m(const VC &c, FT l2_li, FT q) {
    using M = Math<FT>;
    return q > c.eps_1m ? FT(c.vt_k_sno * M::exp2_fin(c.vt_e_sno * l2_li)) : FT(0);
}
// Chen 2022 rain, mass-weighted (k = 3), diameter slope = 2 λ⁻¹ — CM1:251-270, Common.jl:290-302,414-422.  Γ(b+1) from the host-fitted
// polynomials in ρ (NaN fall speed beyond their range, ρ > 2 kg/m³); GENERAL: run-time Γ for parameter sets the fit cannot represent
// l2_rho = log2_floored(ρ⁺) (cmx_math.hpp), shared by the three Chen fall speeds of a point: with it and the floored slope parameter every exponent below is finite
template <typename FT, bool GENERAL = false, typename VC> __device__ __forceinline__ FT vel_rain_chen(const VC &c, FT rp, FT l2_li, FT q, FT l2_rho) {
    using M = Math<FT>;
    const FT l2_lam_inv = l2_li + FT(1);
    const FT lam = M::exp2_fin(-l2_lam_inv);
    const FT l2_q = c.ch_rho0_l2e * rp;
    FT w = FT(0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const FT bi = M::fma(-c.ch_b_rho, rp, c.ch_b[k]);
        FT l2_mag = M::fma(bi, c.l2_1000, l2_q);
        if (k == 2) l2_mag = M::fma(c.ch_a3_pow, l2_rho, l2_mag);
        const FT l2_den = M::log2_pn(lam + c.ch_c1000[k]);                  // λ = 2^finite > 0, c ≥ 0
        const FT e3 = M::exp2_fin(l2_mag - FT(4) * l2_lam_inv - (bi + FT(4)) * l2_den);
        // Γ(b+4)/3!: the fitted polynomial in ρ, or (b+3)(b+2)(b+1)·Γ(b+1)/6 with the run-time Γ
        const FT g = GENERAL ? FT(tgamma_general<FT>(bi + FT(1)) * (bi + FT(3)) * (bi + FT(2)) * (bi + FT(1)) * FT(1.0 / 6.0)) : chen_gamma_eval<typename M::Scalar>(c.chg, k, rp);
        w = k == 0 ? FT((c.ch_a[k] * e3) * g) : M::fma(c.ch_a[k] * e3, g, w);
    }
    w = M::max(FT(0), w);
    if constexpr (!GENERAL) w = rp > FT(kChenGammaRhoMax) ? M::nan() : w;       // outside the range of the fitted Γ: no silent extrapolation
    return q > c.eps_1m ? w : FT(0);
}
template <typename FT, bool GENERAL = false, typename VC> __device__ __forceinline__ FT vel_rain_chen(const VC &c, FT rp, FT l2_li, FT q) {
    return vel_rain_chen<FT, GENERAL>(c, rp, l2_li, q, log2_floored(rp));
}
// CMNonEq.terminal_velocity(::CloudLiquid, ::StokesRegimeVelType, ρ, q): Stokes at the mean-volume diameter — NonEq:250-265
template <typename FT, typename VC> __device__ __forceinline__ FT vel_lcl_stokes(const VC &c, FT rho, FT q) {
    using M = Math<FT>;
    const FT D2 = M::exp2_fin(FT(2.0 / 3.0) * log2_floored(c.st_D3 * rho * M::max(FT(0), q)));
    return q > c.eps_1m ? FT(c.st_pref * (c.st_rho_w * M::rcp(rho) - FT(1)) * D2) : FT(0);
}
// CMNonEq.terminal_velocity(::CloudIce, ::Chen2022VelTypeSmallIce, ρ, q): Σ aₖ D^bₖ e^{−cₖD} at that diameter — NonEq:267-281
template <typename FT, typename VC> __device__ __forceinline__ FT vel_icl_chen(const VC &c, FT rho, FT rp, FT q, FT l2_rho) {
    using M = Math<FT>;
    const FT l2_D = FT(1.0 / 3.0) * log2_floored(c.ci_D3 * rho * M::max(FT(0), q));
    const FT D = M::exp2_fin(l2_D);
    const FT b = M::fma(rp, c.ci_C, c.ci_B);
    const FT common = M::exp2_fin(c.ci_A * l2_rho + b * (c.l2_1000 + l2_D));             // ρₐ^As · (1000 D)^b
    const FT w = common * M::fma(c.ci_F, M::exp2_fin(-c.ci_c2 * D * FT(1.4426950408889634)), c.ci_E);
    return q > c.eps_1m ? FT(M::max(FT(0), w)) : FT(0);
}
template <typename FT, typename VC> __device__ __forceinline__ FT vel_icl_chen(const VC &c, FT rho, FT rp, FT q) {
    return vel_icl_chen<FT>(c, rho, rp, q, log2_floored(rp));
}
// CM1.terminal_velocity(::Snow, ::Chen2022VelTypeLargeIce, ρ, q): mass-weighted (k = 3), λ_D⁻¹ = 2 λ⁻¹ — CM1:272-297
// SHAPED: … with a snow shape (CM1:299-324; VC = Vel1mShapeConsts): ϕ_av^κ = (ϕ₀ Γ)^κ 2^(−κα) (λ_D⁻¹)^(κα) replaces ϕ^κ — the amplitudes and the
// power of term 1 are folded on the host (add_sedimentation_consts), the power of term 2 is the one extra constant sn_e2 = κα − 4
template <typename FT, bool SHAPED = false, typename VC> __device__ __forceinline__ FT vel_snow_chen(const VC &c, FT rp, FT l2_li, FT q, FT l2_rho) {
    using M = Math<FT>;
    const FT l2_ld = l2_li + FT(1), lam = M::exp2_fin(-l2_ld);
    const FT l2_ra = c.sn_A * l2_rho;
    // aₖ e^{−4 ln λ_D⁻¹ − (bₖ+4) ln(λ_D + cₖ)}: term 1 has c = 0 → λ_D^{−b₁}·… collapses to one power
    const FT t1 = c.sn_a1 * M::exp2_fin(l2_ra + c.sn_b1 * l2_ld);
    FT x2 = l2_ra + c.sn_H * rp * FT(1.4426950408889634);
    if constexpr (SHAPED) x2 = x2 + c.sn_e2 * l2_ld;      // sn_e2 = −4 gives the fixed-aspect-ratio value exactly: x − 4l = x + (−4)l in IEEE arithmetic
    else x2 = x2 - FT(4) * l2_ld;
    const FT t2 = c.sn_a2 * M::exp2_fin(x2 - (c.sn_b2 + FT(4)) * M::log2_pn(lam + c.sn_c2));
    return q > c.eps_1m ? FT(M::max(FT(0), t1 + t2)) : FT(0);
}
template <typename FT, bool SHAPED = false, typename VC> __device__ __forceinline__ FT vel_snow_chen(const VC &c, FT rp, FT l2_li, FT q) {
    return vel_snow_chen<FT, SHAPED>(c, rp, l2_li, q, log2_floored(rp));
}
// cmx_snow_terminal_velocity_* per point: the shaped fall speed on the raw (ρ, q) of the point.  ρ⁺ = max(0, ρ) as in the velocity kernel
// (cmx_mp1m_kernels.hip), so that CMX_SNOW_SHAPE_ASPR is bit-identical to its w_sno wherever no input is NaN; a NaN in ρ or q gives NaN (include/cmx.h
// "Conventions"), and in Float64 so does ρ ≤ 0 (bad_density), as in every Float64 1-moment entry
template <typename FT, typename VC> __device__ __forceinline__ FT vel_snow_shaped(const VC &c, FT rho, FT q) {
    using M = Math<FT>;
    const FT rp = M::max(FT(0), rho);
    const FT w = vel_snow_chen<FT, true>(c, rp, vel_l2_li_snow<FT>(c, rp, q), q);
    typename M::Mask bad = nan_mask(rho, q);
    if constexpr (M::IS_F64) bad = (bool)((int)bad | (int)bad_density(rho));
    return bad ? M::nan() : w;
}

// ---- sedimentation fluxes of the fused column step (cmx_mp1m_column.hip) ------------------------------------------------------------
template <typename FT> struct SedFlux4 { FT f[4]; };   // lcl, icl, rai, sno

// F = ρ⁺ χ⁺ w(ρ⁺, χ⁺) of the four species of one raw point
// SHAPED: the snow flux with the shaped fall speed (VC = Vel1mShapeConsts; cmx_mp1m_column_tendencies_sedimentation_* with a CMX_1M_SED_SNOW_* bit)
template <typename FT, bool GENERAL_GAMMA, bool SHAPED = false, typename VC>
__device__ __forceinline__ SedFlux4<FT> mp1m_sed_fluxes(const VC &vc, FT rho, FT q_lcl, FT q_icl, FT q_rai, FT q_sno) {
    using M = Math<FT>;
    const FT r_ = max0(rho), ql = max0(q_lcl), qi = max0(q_icl), qr = max0(q_rai), qs = max0(q_sno);
    SedFlux4<FT> F;
    // one species after the other (consts_after: only one species' constants live where they are read through the kernel-argument pointer)
    F.f[0] = (r_ * ql) * vel_lcl_stokes<FT>(vc, r_, ql);
    const VC &v1 = consts_after(vc, F.f[0]);
    const FT l2_rho = log2_floored(r_);      // once for the three Chen fall speeds
    F.f[1] = (r_ * qi) * vel_icl_chen<FT>(v1, r_, r_, qi, l2_rho);
    const VC &v2 = consts_after(v1, F.f[1]);
    // (the general-Γ instantiation forms its own log2 ρ: with the shared one live across its run-time Γ calls the LinearizedAverage column kernel is left
    // with a 100-byte private segment that no instruction touches — tests/test_kernel_resources.py)
    F.f[2] = (r_ * qr) * vel_rain_chen<FT, GENERAL_GAMMA>(v2, r_, vel_l2_li_rain<FT>(v2, r_, qr), qr, GENERAL_GAMMA ? log2_floored(keep(r_)) : l2_rho);
    const VC &v3 = consts_after(v2, F.f[2]);
    F.f[3] = (r_ * qs) * vel_snow_chen<FT, SHAPED>(v3, r_, vel_l2_li_snow<FT>(v3, r_, qs), qs, l2_rho);
    // NaN in → NaN out per species; Float64: ρ ≤ 0 poisons the point, as in the tendencies (cmx_math.hpp bad_density)
    auto poison = [&](FT q_s, FT f) -> FT {
        typename M::Mask bad = nan_mask(rho, q_s);
        if constexpr (M::IS_F64) bad = (bool)((int)bad | (int)bad_density(rho));
        return bad ? M::nan() : f;
    };
    F.f[0] = poison(q_lcl, F.f[0]); F.f[1] = poison(q_icl, F.f[1]); F.f[2] = poison(q_rai, F.f[2]); F.f[3] = poison(q_sno, F.f[3]);
    return F;
}

// … and the same fluxes TOGETHER WITH the fall speed each one multiplies in (cmx_column_implicit_step.hip: backward-Euler sedimentation needs w itself).
// F is formed by the operations of mp1m_sed_fluxes above on the same operands, so it has its bits (tests/test_column_implicit_step_gpu.py compares them with
// inv_dz = 0); w is the value in registers and is not poisoned: a NaN input reaches the step through F.
template <typename FT> struct SedFluxW4 { FT f[4], w[4]; };   // lcl, icl, rai, sno

template <typename FT, bool GENERAL_GAMMA, typename VC>
__device__ __forceinline__ SedFluxW4<FT> mp1m_sed_fluxes_w(const VC &vc, FT rho, FT q_lcl, FT q_icl, FT q_rai, FT q_sno) {
    using M = Math<FT>;
    const FT r_ = max0(rho), ql = max0(q_lcl), qi = max0(q_icl), qr = max0(q_rai), qs = max0(q_sno);
    SedFluxW4<FT> F;
    F.w[0] = vel_lcl_stokes<FT>(vc, r_, ql);
    F.f[0] = (r_ * ql) * F.w[0];
    const VC &v1 = consts_after(vc, F.f[0]);
    const FT l2_rho = log2_floored(r_);
    F.w[1] = vel_icl_chen<FT>(v1, r_, r_, qi, l2_rho);
    F.f[1] = (r_ * qi) * F.w[1];
    const VC &v2 = consts_after(v1, F.f[1]);
    F.w[2] = vel_rain_chen<FT, GENERAL_GAMMA>(v2, r_, vel_l2_li_rain<FT>(v2, r_, qr), qr, GENERAL_GAMMA ? log2_floored(keep(r_)) : l2_rho);
    F.f[2] = (r_ * qr) * F.w[2];
    const VC &v3 = consts_after(v2, F.f[2]);
    F.w[3] = vel_snow_chen<FT, false>(v3, r_, vel_l2_li_snow<FT>(v3, r_, qs), qs, l2_rho);
    F.f[3] = (r_ * qs) * F.w[3];
    auto poison = [&](FT q_s, FT f) -> FT {
        typename M::Mask bad = nan_mask(rho, q_s);
        if constexpr (M::IS_F64) bad = (bool)((int)bad | (int)bad_density(rho));
        return bad ? M::nan() : f;
    };
    F.f[0] = poison(q_lcl, F.f[0]); F.f[1] = poison(q_icl, F.f[1]); F.f[2] = poison(q_rai, F.f[2]); F.f[3] = poison(q_sno, F.f[3]);
    return F;
}

// The folds below are generic in how a parameter is read and in the scalar the result holds, as make_mp1m_consts_from (cmx_mp1m.hpp): a reader returns a
// field as the working scalar W — double for the plain folds (make_vel1m_consts, add_sedimentation_consts: the double arithmetic they always were), a value
// with a tangent for the parameter derivatives of the column step (cmx_mp1m_column_param.hpp, W = ParamTan; the value parts are the plain fold's in every
// bit).  VC: Vel1mConsts<FT> or a struct with the members the Chen-2022 / Stokes fall speeds read; a member of an arithmetic type holds the value only.
template <typename M, typename W> inline void put_const(M &m, const W &w) {
    if constexpr (std::is_arithmetic<M>::value) m = (M)(double)w;
    else m = (M)w;
}
template <typename VC, typename = void> struct has_blk1m_consts : std::false_type {};
template <typename VC> struct has_blk1m_consts<VC, std::void_t<decltype(std::declval<VC>().vt_k_rai)>> : std::true_type {};

// *chen_general (optional): true when the Chen-2022 rain table needs the GENERAL instantiation (the Γ fit is not accurate for it).  P reads `mp`, C reads
// `*chen`; b and b_ρ of the table are read as values: they reach the fall speed through Γ, which carries no tangent (ChenGamma stays plain).
template <typename FT, typename R, typename VC, typename MP, typename CH, typename PM, typename PC>
static void make_vel1m_consts_from(VC &c, const MP &mp, const CH *chen, bool *chen_general, const PM &P, const PC &C) {
    using W = decltype(P(mp.rain.n0));
    // reuse the folding of the tendencies kernel (thermo part unused): a neutral thermo struct keeps it well-defined
    cmx_thermo_f64 tp{461.5, 287.0, 1004.5, 1859.0, 4181.0, 2070.0, 2.5008e6, 2.8344e6, 273.16, 273.16, 611.657, 273.15, 4181.0};
    const Mp1mConsts<R> m = make_mp1m_consts_from<FT, R>(mp, tp, 0u, (double)Math<FT>::eps_1m(), P, [](const auto &f) { return W((double)f); });
    put_const(c.eps_1m, m.eps_1m); put_const(c.l2_eps, m.l2_eps); put_const(c.lam_a_rai, m.lam_a_rai); put_const(c.lam_b_rai, m.lam_b_rai);
    put_const(c.lam_floor_rai, m.lam_floor_rai); put_const(c.lam_a_sno, m.lam_a_sno); put_const(c.lam_b_sno, m.lam_b_sno);
    put_const(c.lam_floor_sno, m.lam_floor_sno); put_const(c.sno_l2_mu, m.sno_l2_mu); put_const(c.sno_nu, m.sno_nu);
    if constexpr (has_blk1m_consts<VC>::value) {
        put_const(c.rho_w, m.rho_w); put_const(c.vt_k_rai, m.vt_k_rai); put_const(c.vt_e_rai, m.vt_e_rai); put_const(c.vt_k_sno, m.vt_k_sno);
        put_const(c.vt_e_sno, m.vt_e_sno);
    }
    put_const(c.l2_1000, std::log2(1000.0));
    if (chen) {
        put_const(c.ch_rho0_l2e, C(chen->rho_0) * 1.4426950408889634074);
        for (int k = 0; k < 3; ++k) {
            put_const(c.ch_a[k], C(chen->a[k])); put_const(c.ch_b[k], (double)chen->b[k]); put_const(c.ch_c1000[k], C(chen->c[k]) * 1000.0);
        }
        put_const(c.ch_a3_pow, C(chen->a3_pow)); put_const(c.ch_b_rho, (double)chen->b_rho);
        const bool fit_ok = make_chen_gamma<FT>(*chen, c.chg, 3);
        if (chen_general) *chen_general = !fit_ok;
    } else if (chen_general) {
        *chen_general = false;
    }
}
template <typename FT, typename MP, typename CH>
static Vel1mConsts<FT> make_vel1m_consts(const MP &mp, const CH *chen, bool *chen_general = nullptr) {
    Vel1mConsts<FT> c{};
    const auto rd = [](const auto &f) { return (double)f; };
    make_vel1m_consts_from<FT, FT>(c, mp, chen, chen_general, rd, rd);
    return c;
}

// The aspect-ratio factor of the Chen-2022 snow fall speed, as amp · (λ_D⁻¹)^ka with λ_D⁻¹ = 2 λ⁻¹ (λ⁻¹: the radius slope parameter, CM1.lambda_inverse):
//   CMX_SNOW_SHAPE_ASPR     ϕ^κ of the fixed aspect ratio (CM1:287-295): amp = ϕ^κ, ka = 0
//   CMX_SNOW_SHAPE_OBLATE   ϕ_av^κ, ϕ_av = ϕ₀ (λ⁻¹)^α Γ_aspect (CM1:299-324) with CM1.aspect_ratio_coeffs (CM1:155-195):
//   CMX_SNOW_SHAPE_PROLATE    amp = (ϕ₀ Γ_aspect)^κ 2^(−κα), ka = κα
template <typename W> struct SnowAspectOf { W amp, ka; };
using SnowAspect = SnowAspectOf<double>;
template <typename MP, typename PM> static auto snow_aspect_from(const MP &mp, uint32_t shape, const PM &P) {
    using std::exp2; using std::pow; using std::sqrt;
    using W = decltype(P(mp.snow.phi));
    const double pi = 3.14159265358979323846;
    const auto &m = mp.snow.mass;
    const auto &a = mp.snow.area;
    const W ri = P(mp.snow.rho_i), mexp = P(m.me) + P(m.delta_m), aexp = P(a.ae) + P(a.delta_a);
    const W cm = P(m.chi_m) * P(m.m0), ca = P(a.chi_a) * P(a.a0), d0 = 2.0 * P(m.r0);
    W alpha, phi0, kappa, gam;
    if (shape == CMX_SNOW_SHAPE_OBLATE) {            // ϕ(r) = 3√π m(r) / (4 ρᵢ a(r)^{3/2})
        alpha = mexp - 1.5 * aexp;
        phi0 = 3.0 * std::sqrt(pi) / 4.0 / ri * cm / pow(ca, W(1.5)) / pow(d0, alpha);
        kappa = W(1.0 / 3.0);
        gam = P(mp.snow.gamma_aspect_oblate);
    } else if (shape == CMX_SNOW_SHAPE_PROLATE) {    // ϕ(r) = 16 ρᵢ² a(r)³ / (9π m(r)²)
        alpha = 3.0 * aexp - 2.0 * mexp;
        phi0 = 16.0 * ri * ri / 9.0 / pi * pow(ca, W(3.0)) / (cm * cm) / pow(d0, alpha);
        kappa = W(-1.0 / 6.0);
        gam = P(mp.snow.gamma_aspect_prolate);
    } else {
        return SnowAspectOf<W>{pow(P(mp.snow.phi), P(mp.snow.kappa)), W(0.0)};
    }
    const W ka = kappa * alpha;
    return SnowAspectOf<W>{pow(phi0 * gam, kappa) * exp2(-ka), ka};
}
template <typename MP> static SnowAspect snow_aspect(const MP &mp, uint32_t shape) {
    return snow_aspect_from(mp, shape, [](const auto &f) { return (double)f; });
}

// adds the cloud-liquid (Stokes) and Chen-2022 ice constants of the four sedimentation velocities a host model precomputes
// (ClimaAtmos set_sedimentation_precomputed_quantities; test/gpu_clima_core_test.jl:36-45, KA kernel test/gpu_tests.jl:608-630);
// snow_shape (CMX_SNOW_SHAPE_*): the aspect-ratio factor folded into the snow constants (snow_aspect; vel_snow_chen<FT, true> then also
// needs Vel1mShapeConsts::sn_e2 = ka − 4, see make_snow_shape_consts).  P reads `mp`, S `*stokes`, I `*chen_ice`: the Chen-2022 ice tables are reduced at
// the apparent densities in closed form, so every coefficient, ρᵢ and N_0 carry exact tangents (Γ(C_l + 4), Γ(F_l + 4): tgamma of the working scalar).
template <typename FT, typename VC, typename MP, typename ST, typename CI, typename PM, typename PS, typename PI>
static void add_sedimentation_consts_from(VC &c, const MP &mp, const ST *stokes, const CI *chen_ice, uint32_t snow_shape, const PM &P, const PS &S, const PI &I) {
    using std::exp; using std::log; using std::pow; using std::sqrt; using std::tgamma;
    using W = decltype(P(mp.snow.rho_i));
    const double pi = 3.14159265358979323846;
    if (stokes) {
        put_const(c.st_pref, S(stokes->grav) / (18.0 * S(stokes->nu_air)));
        put_const(c.st_rho_w, S(stokes->rho_w));
        put_const(c.st_D3, 6.0 / pi / (P(mp.cloud_liquid.N_0) * P(mp.cloud_liquid.rho_w)));
    }
    if (chen_ice) {
        {   // small ice reduced at the cloud-ice apparent density — Common.jl:304-325
            const auto &t = chen_ice->small_ice;
            const W ri = P(mp.cloud_ice.rho_i), l = log(ri), sq = sqrt(ri);
            put_const(c.ci_D3, 6.0 / pi / (P(mp.cloud_ice.N_0) * ri));
            put_const(c.ci_A, I(t.A[1]) * l * l - I(t.A[2]) * l + I(t.A[0]));
            put_const(c.ci_B, 1.0 / (I(t.B[0]) + I(t.B[1]) * l + I(t.B[2]) / sq));
            put_const(c.ci_C, I(t.C[0]) + I(t.C[1]) * exp(I(t.C[2]) * ri) + I(t.C[3]) * sq);
            put_const(c.ci_E, I(t.E[0]) - I(t.E[1]) * l * l + I(t.E[2]) * sq);
            put_const(c.ci_F, -exp(I(t.F[0]) - I(t.F[1]) * l * l + I(t.F[2]) * l));
            put_const(c.ci_c2, 1000.0 / (I(t.G[0]) + I(t.G[1]) / l - I(t.G[2]) * l / ri));
        }
        {   // large ice reduced at the snow apparent density — Common.jl:327-350; ϕ^κ Γ(b+4)/3! folded in (CM1:287-295)
            const auto &t = chen_ice->large_ice;
            const W ri = P(mp.snow.rho_i), l = log(ri), sq = sqrt(ri);
            const W Al = I(t.A[0]) + I(t.A[1]) * l + I(t.A[2]) / (ri * sq);
            const W Bl = exp(I(t.B[0]) + I(t.B[1]) * l * l + I(t.B[2]) * l);
            const W Cl = exp(I(t.C[0]) + I(t.C[1]) / l + I(t.C[2]) / ri);
            const W El = I(t.E[0]) + I(t.E[1]) * l * sq + I(t.E[2]) * sq;
            const W Fl = I(t.F[0]) + I(t.F[1]) * l - exp(log(-I(t.F[2])) - ri);
            const W Gl = 1.0 / (I(t.G[0]) + I(t.G[1]) * l * sq + I(t.G[2]) / sq);
            const W Hl = I(t.H[0]) + I(t.H[1]) * ri * ri * sq + exp(log(-I(t.H[2])) - ri);
            const auto sa = snow_aspect_from(mp, snow_shape, P);
            const W pk = sa.amp;
            put_const(c.sn_A, Al); put_const(c.sn_b1, Cl + sa.ka); put_const(c.sn_b2, Fl); put_const(c.sn_H, Hl); put_const(c.sn_c2, 1000.0 * Gl);
            put_const(c.sn_a1, pk * Bl * pow(W(1000.0), Cl) * tgamma(Cl + 4.0) / 6.0);
            put_const(c.sn_a2, pk * El * pow(W(1000.0), Fl) * tgamma(Fl + 4.0) / 6.0);
        }
    }
}
template <typename FT, typename MP, typename ST, typename CI>
static void add_sedimentation_consts(Vel1mConsts<FT> &c, const MP &mp, const ST *stokes, const CI *chen_ice, uint32_t snow_shape = CMX_SNOW_SHAPE_ASPR) {
    const auto rd = [](const auto &f) { return (double)f; };
    add_sedimentation_consts_from<FT>(c, mp, stokes, chen_ice, snow_shape, rd, rd, rd);
}

// the constants of cmx_snow_terminal_velocity_* and of the shaped column step: chen_rain / stokes may be NULL (CR / ST name their types)
template <typename FT, typename MP, typename CR, typename ST, typename CI>
static Vel1mShapeConsts<FT> make_snow_shape_consts(const MP &mp, const CR *chen_rain, const ST *stokes, const CI &chen_ice, uint32_t snow_shape,
                                                   bool *chen_general = nullptr) {
    Vel1mShapeConsts<FT> c{};
    static_cast<Vel1mConsts<FT> &>(c) = make_vel1m_consts<FT>(mp, chen_rain, chen_general);
    add_sedimentation_consts<FT>(c, mp, stokes, &chen_ice, snow_shape);
    c.sn_e2 = (FT)(snow_aspect(mp, snow_shape).ka - 4.0);
    return c;
}

}  // namespace cmx
