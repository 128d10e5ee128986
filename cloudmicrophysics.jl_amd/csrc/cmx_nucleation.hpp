// cmx_nucleation.hpp — aerosol nucleation rates (CloudMicrophysics.Nucleation) and the P3 ice-nucleation counts (CMI_het.P3_deposition_N_i /
// P3_het_N_i), per point.  Shared by the streaming kernels of cmx_nucleation_kernels.hip and, under CMX_HOST_BUILD, by the g++ build of
// tests/native/nucleation_host.cpp.
//
// Reference (src = the reference's src/): Nucleation.jl — apparent_nucleation_rate :23-37, h2so4_nucleation_rate :51-90,
// organic_nucleation_rate :106-135, organic_nucleation_rate_hom_prescribed :137-157, organic_and_h2so4_nucleation_rate :172-190,
// organic_and_h2so4_nucleation_rate_bioOxOrg_prescribed :192-206; IceNucleation.jl — P3_deposition_N_i :162-166, P3_het_N_i :202-205.
//
// Every power is evaluated in the log2 domain (x^p = exp2(p·log2 x)) with ONE log2 per base: log2(h2so4/ref) for the four powers of the H2SO4
// concentration, log2(nh3/ref) for the two ^p_A, log2(HOM/ref) for both exponents of the organic rate.  k_{x,y}(T)·(h2so4/ref)^p is one exp2 of the
// summed logarithms (no separate underflow of k or of the power), and the exponent p_t_y·log2(h2so4/ref) is formed once and used in f_y and in the
// ternary term.  f_y's ratio (h2so4/ref)^p_t_y / (nh3/ref)^p_A_y is one exp2 of the exponent difference: (nh3/ref)^p_A_y alone underflows Float32 at
// ordinary ammonia concentrations, the ratio does so only where it is truly below floatmin.
//
// Special values follow IEEE pow as Julia's ^ has them: log2(0) = −Inf gives 0^p = 0 (p > 0), nh3 = 0 gives f_y = 0 and a ternary rate of exactly 0,
// h2so4 = nh3 = 0 gives 0/0 = NaN as in the reference; 1^y = 1 for every y (the apparent rate at output_diam = input_diam; there the ratio is an IEEE division).  A negative base of a
// non-integer power is a DomainError in Julia: here log2 of it is NaN, and the library's rule for a reference DomainError is NaN.  Float64 therefore
// calls the FULL lean forms (exp2 / log2 / rcp, cmx_lean_f64.hpp) throughout: their arguments reach 0, ±Inf and subnormal values here.
#pragma once
#include "cmx_math.hpp"

namespace cmx {

constexpr double kNucLog2e = 1.4426950408889634074;

// host-folded constants (double → FT): see make_nucleation_consts
template <typename FT> struct NucConsts {
    // h2so4_nucleation_rate, index y = 0..3 for (b,n), (b,i), (t,n), (t,i):  log2 k_y(T) = ku_y − log2e · exp2(kv_y T − kw_y)
    FT ku[4], kv[4], kw[4], p[4];        // ku = u log2e, kv = v log2e / 1000, kw = v w log2e; p = p_b_n, p_b_i, p_t_n, p_t_i
    FT pA[2], a[2];                      // f_y, y = n, i: p_A_y, a_y
    // organic: HOM = (yk_o3 2^(e_o3/T) MT O3 + yk_oh 2^(e_oh/T) MT OH) / CS (concentrations ×1e-6), x = HOM/1e7
    FT a1, a2, a3, a4, a5e7, yk_o3, yk_oh, e_o3, e_oh;     // a5e7 = a_5·1e7 (a_5/x = a5e7/HOM); yk = Y·k_MT (double); e = exp_MT·log2e
    // mixed: rate = (c_mix (h2so4·h2so4)) · bioOxOrg_raw with bioOxOrg_raw = k_oh_m 2^(e_oh_m/T) MT OH / CS; prescribed: c_mix_p instead
    FT k_oh_m, e_oh_m, c_mix, c_mix_p;
};

template <typename FT, typename HP, typename OP, typename MP>
inline NucConsts<FT> make_nucleation_consts(const HP *h, const OP *o, const MP *m) {
    NucConsts<FT> c{};
    const double l2e = kNucLog2e;
    if (h) {
        const double u[4] = {h->u_b_n, h->u_b_i, h->u_t_n, h->u_t_i}, v[4] = {h->v_b_n, h->v_b_i, h->v_t_n, h->v_t_i},
                     w[4] = {h->w_b_n, h->w_b_i, h->w_t_n, h->w_t_i}, p[4] = {h->p_b_n, h->p_b_i, h->p_t_n, h->p_t_i};
        for (int y = 0; y < 4; ++y) {
            c.ku[y] = (FT)(u[y] * l2e);
            c.kv[y] = (FT)(v[y] * l2e / 1000.0);
            c.kw[y] = (FT)(v[y] * w[y] * l2e);
            c.p[y] = (FT)p[y];
        }
        c.pA[0] = (FT)h->p_A_n; c.pA[1] = (FT)h->p_A_i;
        c.a[0] = (FT)h->a_n; c.a[1] = (FT)h->a_i;
    }
    if (o) {
        c.a1 = (FT)o->a_1; c.a2 = (FT)o->a_2; c.a3 = (FT)o->a_3; c.a4 = (FT)o->a_4; c.a5e7 = (FT)((double)o->a_5 * 1e7);
        c.yk_o3 = (FT)((double)o->Y_MTO3 * (double)o->k_MTO3); c.yk_oh = (FT)((double)o->Y_MTOH * (double)o->k_MTOH);
        c.e_o3 = (FT)((double)o->exp_MTO3 * l2e); c.e_oh = (FT)((double)o->exp_MTOH * l2e);
    }
    if (m) {
        c.k_oh_m = (FT)m->k_MTOH; c.e_oh_m = (FT)((double)m->exp_MTOH * l2e);
        // :172-206: bioOxOrg ×1e6 then ×1e-6, k_H2SO4org ×1e-6 and the result ×1e6 cancel pairwise; the prescribed form keeps one 1e-6
        c.c_mix = (FT)(0.5 * (double)m->k_H2SO4org);
        c.c_mix_p = (FT)(0.5e-6 * (double)m->k_H2SO4org);
    }
    return c;
}

// 2^t for a term that is multiplied up afterwards (by an ion concentration, f_y, the 1e6 unit factor): Float32 returns 2^(t+64) with unscale = 2^-64
// where t < −64, so that the product keeps full precision where 2^t alone would be subnormal — the hardware exp2 flushes those to 0, while k·x^p·ion
// is still ≫ floatmin — and the caller multiplies by `unscale` last, after the unit factor 1e6.  Scaling by powers of two is exact: the result is the unscaled one wherever
// that does not underflow, and nothing overflows that did not before.  Float64 keeps 2^t (its subnormals lie far below every rate).
template <typename FT> __device__ __forceinline__ FT exp2_scaled(FT t, FT &unscale) {
    using M = Math<FT>;
    if constexpr (M::IS_F64) {
        unscale = FT(1);
        return M::exp2(t);
    } else {
        const bool lo = t < FT(-64);
        unscale = lo ? FT(5.421010862427522e-20) : FT(1);          // 2^-64
        return M::exp2(lo ? t + FT(64) : t);
    }
}

// h2so4_nucleation_rate — Nucleation.jl:51-90.  h2so4 and nh3 in m⁻³ (scaled ×1e-6 to cm⁻³ and by the reference 1e6 cm⁻³: log2(1e-12) added to their
// logarithms), negative_ion in m⁻³ UNSCALED (:60-61 scale only h2so4 and nh3), T in K; rates in m⁻³ s⁻¹.  The sums and the final ×1e6 in the
// reference's order (the ×1e6 distributed over the
// terms).  nh3 < 0 makes the reference throw for the whole call (its ^p_A_y): binary is NaN then as well.
template <typename FT, typename C>
__device__ __forceinline__ void h2so4_rates(const C &c, FT h2so4, FT nh3, FT ion, FT T, FT &binary, FT &ternary) {
    using M = Math<FT>;
    const FT L2E = FT(kNucLog2e), L12 = FT(-39.863137138648348);     // log2(1e-12)
    const FT l2x = M::log2(h2so4) + L12, l2z = M::log2(nh3) + L12;     // full log2: 0 → −Inf, < 0 → NaN
    FT lk[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) lk[y] = c.ku[y] - L2E * M::exp2(M::fma(c.kv[y], T, -c.kw[y]));
    FT un, ui, un_t, ui_t;                                               // exp2_scaled: the multiplied-up terms keep their precision below floatmin
    const FT bn = exp2_scaled(M::fma(c.p[0], l2x, lk[0]), un);          // k_b_n (h2so4/ref)^p_b_n
    const FT bi = exp2_scaled(M::fma(c.p[1], l2x, lk[1]), ui);
    const FT ptn = c.p[2] * l2x, pti = c.p[3] * l2x;                     // p_t_y log2(h2so4/ref): f_y and the ternary term
    const FT z = nh3 * FT(1e-12);
    const FT fn = M::div(z, c.a[0] + M::exp2(M::fma(-c.pA[0], l2z, ptn)));
    const FT fi = M::div(z, c.a[1] + M::exp2(M::fma(-c.pA[1], l2z, pti)));
    // the final ×1e6 is distributed over the terms so that `unscale` comes after it (a scaled term is unscaled where it is largest)
    const FT tn = ((fn * exp2_scaled(ptn + lk[2], un_t)) * FT(1e6)) * un_t, ti = (((fi * exp2_scaled(pti + lk[3], ui_t)) * ion) * FT(1e6)) * ui_t;
    const FT b = (bn * FT(1e6)) * un + ((bi * ion) * FT(1e6)) * ui;
    binary = nh3 < FT(0) ? M::nan() : b;
    ternary = tn + ti;
}

// organic_nucleation_rate_hom_prescribed — Nucleation.jl:137-157: HOM in cm⁻³, ion as the function receives it (the composed rate passes ×1e-6).
// x = HOM/1e7: log2 x = log2 HOM + log2(1e-7) once for both exponents, a_5/x = (a_5·1e7)/HOM.
template <typename FT, typename C> __device__ __forceinline__ FT organic_from_hom(const C &c, FT ion, FT hom) {
    using M = Math<FT>;
    const FT l2x = M::log2(hom) + FT(-23.253496664211536);               // log2(1e-7)
    const FT q = M::rcp(hom);
    FT u1, u2;
    const FT p1 = exp2_scaled(M::fma(c.a5e7, q, c.a2) * l2x, u1), p2 = exp2_scaled(M::fma(c.a5e7, q, c.a4) * l2x, u2);
    return ((c.a1 * p1) * FT(1e6)) * u1 + (((c.a3 * p2) * ion) * FT(1e6)) * u2;    // ×1e6 before the unscale, as in h2so4_rates
}

// organic_nucleation_rate — Nucleation.jl:106-135: all four concentrations ×1e-6 (:117-120), products in the reference's order.
// rT = 1/T and rcs = 1/CS are shared with the mixed rate.
template <typename FT, typename C>
__device__ __forceinline__ FT organic_rate(const C &c, FT ion, FT mt, FT o3, FT oh, FT rT, FT rcs) {
    using M = Math<FT>;
    const FT ko3 = c.yk_o3 * M::exp2(c.e_o3 * rT), koh = c.yk_oh * M::exp2(c.e_oh * rT);
    const FT s = FT(1e-6), mts = mt * s;
    const FT hom = (ko3 * mts * (o3 * s) + koh * mts * (oh * s)) * rcs;
    return organic_from_hom<FT>(c, ion * s, hom);
}

// organic_and_h2so4_nucleation_rate — Nucleation.jl:172-190 with :192-206: h2so4 squared UNSCALED (:202 is commented out); MT, OH in m⁻³ unscaled
template <typename FT, typename C>
__device__ __forceinline__ FT mixed_rate(const C &c, FT h2so4, FT mt, FT oh, FT rT, FT rcs) {
    using M = Math<FT>;
    const FT k = c.k_oh_m * M::exp2(c.e_oh_m * rT);
    const FT bio = ((k * mt) * oh) * rcs;
    return (c.c_mix * (h2so4 * h2so4)) * bio;
}
// organic_and_h2so4_nucleation_rate_bioOxOrg_prescribed — Nucleation.jl:192-206 (bioOxOrg in m⁻³)
template <typename FT, typename C> __device__ __forceinline__ FT mixed_from_bio(const C &c, FT h2so4, FT bio) {
    return (c.c_mix_p * (h2so4 * h2so4)) * bio;
}

// apparent_nucleation_rate — Nucleation.jl:23-37.  The two ratios are IEEE (correctly rounded) divisions, so equal arguments give exactly 1: at
// output_diam = input_diam, 1^(m+1) = 1 for every m (IEEE pow, Julia's ^), γ = (1/±Inf)·0 = 0 and J_x = nucleation_rate exactly — exp2(Inf·log2 1)
// would be NaN — and at coag_sink = coag_sink_input_diam as well m = 0/0 = NaN as in the reference.  log(a)/log(b) = log2(a)/log2(b).
// (r^(m+1) − 1)/(m+1) is evaluated as expm1((m+1) ln r)/(m+1): the reference's difference cancels where m → −1 (a smooth point of γ, whose limit is
// ln r) — 1 % off in Float32 at |m + 1| ≈ 2e-5 — the expm1 form keeps the relative accuracy (as P3_het_N_i below).  r = 1 or m + 1 = 0: 0 (1^y = x^0 = 1).
template <typename FT>
__device__ __forceinline__ FT apparent_rate(FT od, FT nr, FT gr, FT cs, FT csi, FT id) {
    using M = Math<FT>;
    const FT r = od / id;
    const FT l2r = M::log2(r);
    const FT m1 = M::div(M::log2(cs / csi), l2r) + FT(1);
    const FT em1 = (r == FT(1) || m1 == FT(0)) ? FT(0) : M::expm1((m1 * l2r) * FT(0.69314718055994530942));
    const FT g = M::rcp(m1) * em1;
    return nr * M::exp2(M::div((-g * id) * csi, gr) * FT(kNucLog2e));
}

// CMP.MorrisonMilbrandt2014 folded for P3_deposition_N_i / P3_het_N_i
template <typename FT> struct P3NucConsts { FT T_dep, T0, A, c2l, het_B, het_al; };     // A = 1000 c₁, c2l = c₂ log2e, het_al = het_a log2e
template <typename FT, typename IP> inline P3NucConsts<FT> make_p3_nucleation_consts(const IP &ip) {
    return P3NucConsts<FT>{(FT)ip.T_dep_thres, (FT)ip.T0, (FT)(1000.0 * (double)ip.c1), (FT)((double)ip.c2 * kNucLog2e), (FT)ip.het_B,
                           (FT)((double)ip.het_a * kNucLog2e)};
}
// P3_deposition_N_i — IceNucleation.jl:162-166.  A NaN T gives NaN (the library's NaN rule); the reference's ifelse(T < T₀, …, 0) returns 0 there.
template <typename FT, typename C> __device__ __forceinline__ FT p3_deposition_N_i(const C &c, FT T) {
    using M = Math<FT>;
    const FT n = c.A * M::exp2(c.c2l * (c.T0 - M::max(c.T_dep, T)));
    return T != T ? M::nan() : (T < c.T0 ? n : FT(0));
}
// P3_het_N_i — IceNucleation.jl:202-205 as −N_l·expm1(x) in both precisions: the reference's N_l (1 − exp(x)) cancels for |x| ≪ 1 (13 % off in
// Float32 at its own GPU test state), expm1 keeps the relative accuracy.  x = ((−het_B V_l) Δt) exp(het_a Tₛ) in the reference's order.
template <typename FT, typename C> __device__ __forceinline__ FT p3_het_N_i(const C &c, FT T, FT Nl, FT Vl, FT dt) {
    using M = Math<FT>;
    const FT x = ((-c.het_B * Vl) * dt) * M::exp2(c.het_al * (c.T0 - T));
    return -Nl * M::expm1(x);
}

}  // namespace cmx
