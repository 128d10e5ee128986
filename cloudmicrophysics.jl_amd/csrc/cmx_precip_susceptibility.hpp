// cmx_precip_susceptibility.hpp — SB2006 precipitation susceptibilities (CloudMicrophysics.PrecipitationSusceptibility), per point: the logarithmic
// derivatives of the autoconversion and accretion rain source with respect to ln q_lcl, ln q_rai and ln N_lcl.  Shared by the streaming kernel of
// cmx_precip_susceptibility_kernels.hip and, under CMX_HOST_BUILD, by the g++ build of tests/native/precip_susceptibility_host.cpp.
//
// Reference (src = the reference's src/): PrecipitationSusceptibility.jl — precipitation_susceptibility_autoconversion :36-51,
// precipitation_susceptibility_accretion :66-79 — ForwardDiff gradients of ln(dq_rai_dt) of CM2.autoconversion (Microphysics2M.jl:396-427) and
// CM2.accretion (:445-470) with respect to the logarithms of |q_lcl|, |q_rai|, |ρ|, |N_lcl|; components 1, 2 and 4 are returned and d_ln_N_rai is
// always 0.  The gradients have closed forms (the reference's own test writes them down, test/precipitation_susceptibility_tests.jl:11-29,59-68), which
// is what is coded here: no dual numbers on the device.
//
// With ϵ = eps(FT), 1−τ = q_lcl/(q_lcl+q_rai), τ = q_rai/(q_lcl+q_rai) (both as quotients: neither cancels), x̄_c = ρ q_lcl/N_lcl, w = 1 − τ^a:
//   autoconversion   u = A τ^a w^b/(1−τ)²,   G = u/(1+u)·[a − a b τ^a/w + 2τ/(1−τ)],   G = 0 where q_rai < ϵ (the ifelse of :411)
//                    S_q_rai = (1−τ) G;   x̄_c < x_star: S_q_lcl = 4 − S_q_rai, S_N_lcl = −2;   otherwise (the min of :406 clips): S_q_lcl = 2 − S_q_rai, S_N_lcl = 0
//   accretion        h = (1−τ) c τ0/(τ+τ0),   S_q_lcl = 1 − h,   S_q_rai = 1 + h,   S_N_lcl = 0
// (1−τ) G is evaluated with ONE division and none by w:
//   (1−τ) G = A τ^a w^(b−1) [a (1−τ) w − a b τ^a (1−τ) + 2 τ w] / ((1−τ)² + A τ^a w^b)
// so that τ → 1, where w and 1−τ vanish together, gives the finite limit instead of 0·Inf.  b = 3 (the published scheme) takes w^(b−1) = w·w.
//
// NaN contract (cmx's own: the reference was not run): where the reference zeroes dq_rai_dt — autoconversion: q_lcl < ϵ or N_lcl < ϵ; accretion: those or
// q_rai < ϵ — the derivative of the logarithm of that zero is undefined (default ForwardDiff gives 0·Inf = NaN), and all three outputs of that
// process are NaN.  They are NaN as well where an input is NaN or ρ = 0.  The inputs enter through their absolute values, as in the reference.
#pragma once
#include "cmx_math.hpp"

namespace cmx {

template <typename FT> struct SuscConsts {
    FT x_star, A, a, ab, bm1, c_tau0, tau_0;       // ab = a·b, bm1 = b − 1, c_tau0 = c·τ0 (products formed in double)
    int32_t b_is_3;                                // (1 − τ^a)^(b−1) by multiplication (the test sb_integer_exponents makes for b, cmx_sb2006.hpp)
};

template <typename FT, typename AC, typename AR> inline SuscConsts<FT> make_susceptibility_consts(const AC *acnv, const AR *accr) {
    SuscConsts<FT> c{};
    if (acnv) {
        c.x_star = (FT)acnv->x_star; c.A = (FT)acnv->A; c.a = (FT)acnv->a;
        c.ab = (FT)((double)acnv->a * (double)acnv->b); c.bm1 = (FT)((double)acnv->b - 1.0);
        c.b_is_3 = acnv->b == 3;
    }
    if (accr) { c.c_tau0 = (FT)((double)accr->c * (double)accr->tau_0); c.tau_0 = (FT)accr->tau_0; }
    return c;
}

template <typename FT> struct Susceptibilities { FT au_q_lcl, au_q_rai, au_N_lcl, ac_q_lcl, ac_q_rai, ac_N_lcl; };

template <typename FT> __device__ __forceinline__ FT susc_abs(FT x) {
    if constexpr (sizeof(FT) == 8) return __builtin_fabs(x);
    else return __builtin_fabsf(x);
}

// 1 − τ^a where τ → 1: formed from 1 − τ itself, w = −expm1(a ln(1 − (1−τ))), with the two Taylor series below |x| = 1/32 (relative truncation
// error < 1e-8 with 5 terms in Float32, < 1e-17 with 11 / 10 in Float64).  1 − exp2(a log2 τ) loses eps/(a (1−τ)) of w there — 0.4 % in Float32 at
// q_lcl = ϵ under q_rai = 5e-3 — which S_q_rai carries in full once b < 3 (u ∝ (1−τ)^(b−2) is then no longer small).
template <typename FT> __device__ __forceinline__ FT susc_ln1m_small(FT x) {           // ln(1 − x) = −x (1 + x/2 + x²/3 + …), 0 ≤ x < 1/32
    constexpr int N = sizeof(FT) == 8 ? 11 : 5;
    FT s = FT(1.0 / N);
#pragma unroll
    for (int k = N - 1; k >= 1; --k) s = Math<FT>::fma(s, x, FT(1.0 / k));
    return -x * s;
}
template <typename FT> __device__ __forceinline__ FT susc_expm1_small(FT y) {          // e^y − 1 = y (1 + y/2! + y²/3! + …), |y| < 1/32
    constexpr int N = sizeof(FT) == 8 ? 10 : 5;
    double f = 1.0;
    for (int k = 2; k <= N; ++k) f *= k;
    FT s = FT(1.0 / f);
#pragma unroll
    for (int k = N - 1; k >= 1; --k) {
        f /= (k + 1);
        s = Math<FT>::fma(s, y, FT(1.0 / f));
    }
    return y * s;
}

// AU / AC: which process is evaluated (run-time flags, uniform over the launch); the fields of the other are left at 0.
template <typename FT, typename C>
__device__ __forceinline__ Susceptibilities<FT> precip_susceptibility_point(const C &c, bool AU, bool AC, FT q_lcl_in, FT q_rai_in, FT rho_in, FT N_lcl_in) {
    using M = Math<FT>;
    const FT eps = FT(M::eps());                      // ϵ_numerics_2M_M = ϵ_numerics_2M_N = eps(FT)  (Utilities.jl:325,332)
    const FT q_lcl = susc_abs(q_lcl_in), q_rai = susc_abs(q_rai_in), rho = susc_abs(rho_in), N_lcl = susc_abs(N_lcl_in);
    const bool bad = any_nan(q_lcl, q_rai, rho, N_lcl) || rho == FT(0);
    const bool no_q_rai = q_rai < eps;
    const bool gate_au = q_lcl < eps || N_lcl < eps;
    const FT inv_sum = M::rcp(q_lcl + q_rai);
    const FT tau = q_rai * inv_sum, omt = q_lcl * inv_sum;
    Susceptibilities<FT> s{};
    if (AU) {
        const FT ta = M::exp2(c.a * M::log2(tau));                    // τ = 0: log2 = −Inf, τ^a = 0
        const FT y = c.a * susc_ln1m_small<FT>(omt);                 // a ln τ where 1 − τ < 1/32
        const FT w = (omt < FT(0.03125) && y > FT(-0.03125)) ? -susc_expm1_small<FT>(y) : FT(1) - ta;
        const FT wp = c.b_is_3 ? w * w : M::exp2(c.bm1 * M::log2(w));   // w^(b−1)
        const FT k = (c.A * ta) * wp;
        const FT br = M::fma(FT(2) * tau, w, (c.a * omt) * w - (c.ab * ta) * omt);
        const FT G1 = no_q_rai ? FT(0) : M::div(k * br, M::fma(k, w, omt * omt));
        const bool clipped = !(rho * q_lcl < c.x_star * N_lcl);       // x̄_c = ρ q_lcl/N_lcl ≥ x_star, without the division
        const bool nan_au = bad || gate_au;
        s.au_q_rai = nan_au ? M::nan() : G1;
        s.au_q_lcl = nan_au ? M::nan() : (clipped ? FT(2) : FT(4)) - G1;
        s.au_N_lcl = nan_au ? M::nan() : (clipped ? FT(0) : FT(-2));
    }
    if (AC) {
        const FT h = (omt * c.c_tau0) * M::rcp(tau + c.tau_0);
        const bool nan_ac = bad || gate_au || no_q_rai;
        s.ac_q_lcl = nan_ac ? M::nan() : FT(1) - h;
        s.ac_q_rai = nan_ac ? M::nan() : FT(1) + h;
        s.ac_N_lcl = nan_ac ? M::nan() : FT(0);
    }
    return s;
}

}  // namespace cmx
