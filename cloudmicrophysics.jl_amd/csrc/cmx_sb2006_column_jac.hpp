// cmx_sb2006_column_jac.hpp — what the device entries (cmx_sb2006_column_products.hip) and the host test build (tests/native/column_products_host.cpp,
// CMX_HOST_BUILD) share of the products J v and Jᵀḡ with the Jacobian of the SB2006 COLUMN step (include/cmx.h §(25)): the scheme SbColJac — the clamps, the
// point function sb2006_point WITH its fall speeds and the sedimentation fluxes of cmx_sb2006_sed.hpp on the dual value type (cmx_dual.hpp) — its set-up from
// the parameter structs, the argument structs, and the bodies of one point.  No HIP in here.
//
// The function that is differentiated, per column (level 0 lowest, x_k = (T, q_tot, q_lcl, n_lcl, q_rai, n_rai)_k; ρ and inv_dz are held fixed):
//     out_k = tend(ρ_k, x_k) + g_k·(F_{k+1} − F_k),   g_k = inv_dz[k]·(1/ρ_k⁺),   F_{n_lev} = 0,   precip = F_0[q_rai]
// F_k = ρ⁺χ⁺w: the fluxes of q_rai and n_rai, and of q_lcl and n_lcl with cloud sedimentation; F_k depends on x_k only, so the block Jacobian is upper
// bidiagonal in the level index.  With Ḟ_k = (∂F_k/∂x_k)·v_k:
//     J v:   ẏ_k = J_pt(x_k)·v_k + g_k·(Ḟ_{k+1} − Ḟ_k),   ṗ = Ḟ_0[q_rai]
//     Jᵀḡ:   x̄_k = J_pt(x_k)ᵀ·ḡ_k + (∂F_k/∂x_k)ᵀ·λ_k,   λ_k[s] = −g_k·ḡ_k[s] + [k>0]·g_{k−1}·ḡ_{k−1}[s] + [k=0, s=q_rai]·p̄
// The VALUE parts are formed by the operations of sb2006_column_kernel (cmx_sb2006_column.hip) in its order — A = fma(−F, g, sum), then fma(F_above, g, A) below
// the top — so requested tendencies and the precipitation flux are that entry's, bit for bit; the tangents take the same two fma.
#pragma once
#include <cstdint>
#include <type_traits>

#include "../../include/cmx.h"
#include "cmx_column_products.hpp"
#include "cmx_dispatch.hpp"
#include "cmx_jacobian.hpp"
#include "cmx_sb2006.hpp"
#include "cmx_sb2006_sed.hpp"

namespace cmx {

// Tangents per evaluation of the point function in the Jᵀḡ kernel: tuning numbers (-DCMX_COL_VJP_K_F32=…, -DCMX_COL_VJP_K_F64=…, -DCMX_COL_VJP_K_F64_GEN=…),
// the widest that no instantiation spills a VGPR at (VGPRs over the 24 instantiations of a float type, cross-compiled for gfx950):
//     Float32   K = 1: 160–219    K = 2: 174–232    K = 3: 187–246     all at two waves per SIMD, none spills: 3 (two passes for the six inputs)
//     Float64   SB2006 and fitted Chen-2022 fall speeds   K = 1: 288–394    K = 2: 326–438    K = 3: 354–478     none spills: 3
//               general Chen-2022 (run-time Γ)            K = 1: 472–496    K = 2: 510–512, up to 42 spilled    K = 3: 512, 26–62 spilled: 1
// A gradient's bits do not depend on K.
// J v carries the caller's one tangent.
#ifndef CMX_COL_VJP_K_F32
#define CMX_COL_VJP_K_F32 3
#endif
#ifndef CMX_COL_VJP_K_F64
#define CMX_COL_VJP_K_F64 3
#endif
#ifndef CMX_COL_VJP_K_F64_GEN
#define CMX_COL_VJP_K_F64_GEN 1
#endif
template <typename FT, int VEL> constexpr int kColVjpK = sizeof(FT) == 4 ? CMX_COL_VJP_K_F32 : (VEL == VEL_CHEN_GEN ? CMX_COL_VJP_K_F64_GEN : CMX_COL_VJP_K_F64);

// The column scheme of point x = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai): SbJac's four sums (cmx_sb2006_jacobian.hpp) from the point function WITH the
// fall speeds, the four fluxes the point sends down, and g.  Flux slot s: 0 q_rai, 1 n_rai, 2 q_lcl, 3 n_lcl (the members of SedFlux); FLUX_OUT[s] is the
// output whose tendency the flux enters.  Without cloud sedimentation the slots 2 and 3 are constant zeros and NFLUX = 2 of them are used.
template <bool LIMITED, int VEL, bool CLOUD, bool INTPOW> struct SbColJac {
    static constexpr int NOUT = CMX_SB2006_JAC_NOUT, NWRT = CMX_SB2006_JAC_NWRT, NFLUX = CLOUD ? 4 : 2;
    static constexpr bool limited = LIMITED, cloud = CLOUD, intpow = INTPOW;
    static constexpr int vel = VEL;
    static constexpr int flux_out(int s) {
        return s == 0 ? CMX_SB2006_JAC_DQ_RAI_DT : s == 1 ? CMX_SB2006_JAC_DN_RAI_DT : s == 2 ? CMX_SB2006_JAC_DQ_LCL_DT : CMX_SB2006_JAC_DN_LCL_DT;
    }
    // The NaN rule of the primal entry, as selects (−0 stays −0): a NaN in any input poisons the point's outputs; the fluxes depend on
    // (ρ, q_lcl, n_lcl, q_rai, n_rai) only, and a NaN in one of those reaches the cell below through them
    template <typename FT> static __device__ __forceinline__ bool poison(const FT (&x)[NWRT + 1]) { return any_nan(x[0], x[2], x[3], x[4], x[5], x[6], x[1]); }
    template <typename FT> static __device__ __forceinline__ bool flux_poison(const FT (&x)[NWRT + 1]) { return any_nan(x[0], x[3], x[4], x[5], x[6]); }
    template <typename FT> static __device__ __forceinline__ FT out(FT v, bool poison) { return poison ? Math<FT>::nan() : v; }
    // 1/ρ⁺ as the point function forms it (cmx_sb2006.hpp: one reciprocal square root, squared)
    template <typename FT> static __device__ __forceinline__ FT inv_rho(FT rho) {
        const FT rs = Math<FT>::rsqrt(max0(rho));
        return rs * rs;
    }
    // in: the six differentiated inputs in the order of cmx_sb2006_jac_wrt; o: the point sums, F: the fluxes, g = inv_dz·(1/ρ⁺)
    // (CV: CloudVelConsts<FT>, or CloudVelConsts<Dual<FT, K>> next to constants that hold duals themselves: cmx_sb2006_column_param.hpp)
    template <typename FT, int K, typename C, typename CV>
    static __device__ __forceinline__ void eval(const C &c, const CV &cv, FT rho, FT inv_dz, const Dual<FT, K> (&in)[NWRT], Dual<FT, K> (&o)[NOUT],
                                                Dual<FT, K> (&F)[4], FT &g) {
        using D = Dual<FT, K>;
        using MD = Math<D>;
        // clamp_to_nonneg — BMT:828-837 (T is not clamped); the clamps are part of the differentiated function.  ρ is a constant: not differentiated
        const D r_ = D(max0(rho));
        const D T = in[CMX_SB2006_JAC_WRT_T];
        const D qt = max0(in[CMX_SB2006_JAC_WRT_Q_TOT]), ql = max0(in[CMX_SB2006_JAC_WRT_Q_LCL]), nl = max0(in[CMX_SB2006_JAC_WRT_N_LCL]);
        const D qr = max0(in[CMX_SB2006_JAC_WRT_Q_RAI]), nr = max0(in[CMX_SB2006_JAC_WRT_N_RAI]);
        const SbRates<D> p = sb2006_point<D, LIMITED, VEL, false, INTPOW>(scheme_consts<FT>(c), r_, T, qt, ql, qr, r_ * nl, r_ * nr, nl, nr);
        const SedFlux<D> f = sed_fluxes<D, CLOUD>(cv, r_, ql, nl, qr, nr, p.vt_n, p.vt_m);
        F[0] = f.q_rai;
        F[1] = f.n_rai;
        F[2] = f.q_lcl;
        F[3] = f.n_lcl;
        g = inv_dz * p.inv_rho.v;                                          // 1/(ρ_k Δz_k)
        o[CMX_SB2006_JAC_DQ_LCL_DT] = (p.cond + p.au_dq_lcl) + p.ac_dq_lcl;
        o[CMX_SB2006_JAC_DN_LCL_DT] = MD::fma(p.lsc_plus_au + p.ac_dN_lcl, p.inv_rho, p.na_lcl);
        o[CMX_SB2006_JAC_DQ_RAI_DT] = (p.evq + p.au_dq_rai) + p.ac_dq_rai;
        o[CMX_SB2006_JAC_DN_RAI_DT] = MD::fma(((p.evN + p.au_dN_rai) + p.rsc) + p.rbr, p.inv_rho, p.na_rai);
    }
    // the VALUE of the fluxes of a raw point: the primal's flux-only evaluation (the cell above, when Jᵀḡ is asked for the tendencies)
    template <typename FT, typename C>
    static __device__ __forceinline__ SedFlux<FT> flux_values(const C &c, const CloudVelConsts<FT> &cv, FT rho, FT q_lcl, FT n_lcl, FT q_rai, FT n_rai) {
        return sed_fluxes_of_point<FT, LIMITED, VEL, CLOUD>(front_consts<FT>(c), cv, rho, q_lcl, n_lcl, q_rai, n_rai);
    }
};

// The constants of the column scheme as ONE by-value kernel argument, the first (cmx_column_products.hpp): `c` comes first, where front_consts reads it.
// T: FT, or Dual<FT, KP> for the parameter derivatives (cmx_sb2006_column_param.hpp).
template <typename T> struct SbColConsts {
    SbConsts<T> c;
    CloudVelConsts<T> cv;
};

// The statuses of the primal entry's flag checks: no unknown bit, exactly one rain fall-speed scheme
inline int32_t sb2006_column_flags_status(uint32_t flags) {
    if (flags & ~(uint32_t)(CMX_SB2006_LIMITED | CMX_VEL_SB2006 | CMX_VEL_CHEN2022)) return CMX_ERR_BAD_ARG;
    const bool sbv = flags & CMX_VEL_SB2006, chv = flags & CMX_VEL_CHEN2022;
    return sbv == chv ? CMX_ERR_BAD_ARG : CMX_OK;
}

// The set-up the device entries and the host mirror share after the flag, count and column checks: the limiter and fall-speed checks of the primal entry, the
// constants, and the instantiation that entry selects for the same parameter structs.  Returns f(c, cv, SbColJac<…>{}) or CMX_ERR_BAD_ARG.
template <typename FT, typename WR, typename TH, typename VL, typename ST, typename F>
inline int32_t with_sb2006_column_jac(const WR &wr, const TH &tps, const VL &vel, const ST *cloud_vel, uint32_t flags, F &&f) {
    const bool limited = flags & CMX_SB2006_LIMITED, sbv = flags & CMX_VEL_SB2006;
    if (limited && !sb_limiters_ok(wr)) return CMX_ERR_BAD_ARG;      // clamp_ordered needs ordered limiter pairs
    if (sbv && !sb_rain_vel_ok(vel, limited)) return CMX_ERR_BAD_ARG;      // the not-limited SB2006 fall speed needs aR < bR
    const SbConsts<FT> c = make_sb_consts<FT>(wr, tps, &vel, (double)Math<FT>::eps_1m());
    CloudVelConsts<FT> cv{};
    if (cloud_vel) cv = make_cloud_vel_consts<FT>(wr.seifert_beheng.pdf_c, *cloud_vel);
    const int velk = sbv ? VEL_SB : chen_vel_kind<FT>(vel.chen2022);   // fitted Γ(b(ρ)+1) or the general instantiation (cmx_math.hpp ChenGamma)
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG,
                       [&](auto L, auto V, auto CL, auto I) -> int32_t {
                           return f(c, cv, SbColJac<decltype(L)::value, decltype(V)::value, decltype(CL)::value, decltype(I)::value>{});
                       },
                       flag(limited), one_of<VEL_SB, VEL_CHEN, VEL_CHEN_GEN>(velk), flag(cloud_vel != nullptr), flag(sb_integer_exponents(wr)));
}

// ---- J v ------------------------------------------------------------------------------------------------------------------------------------------
// `tan[j]`: the tangent column of differentiated input j (NULL: zero).  `jvp[q]`, `tend[q]`: n values each; `jvp_precip`, `precip`: one per column.  All NULL-able.
template <typename FT> struct ColJvpArgs {
    const FT *in[CMX_SB2006_JAC_NWRT + 1];      // rho, then the differentiated inputs
    const FT *tan[CMX_SB2006_JAC_NWRT];
    FT *jvp[CMX_SB2006_JAC_NOUT];
    FT *tend[CMX_SB2006_JAC_NOUT];
    FT *jvp_precip, *precip;
    const FT *inv_dz;
    int64_t n;                                   // n_col · n_lev
    int32_t n_lev;
};

// False if the call has no output at all
template <typename FT>
inline bool make_col_jvp_args(ColJvpArgs<FT> &a, const FT *const (&in)[CMX_SB2006_JAC_NWRT + 1], const FT *inv_dz, int64_t n, int32_t n_lev, const FT *const *tangents,
                              FT *const *jvp, FT *jvp_precip, FT *const *tendencies, FT *precip) {
    a = ColJvpArgs<FT>{};
    for (int j = 0; j < CMX_SB2006_JAC_NWRT + 1; ++j) a.in[j] = in[j];
    for (int j = 0; j < CMX_SB2006_JAC_NWRT; ++j) a.tan[j] = tangents ? tangents[j] : nullptr;
    bool any = jvp_precip != nullptr || precip != nullptr;
    for (int q = 0; q < CMX_SB2006_JAC_NOUT; ++q) {
        a.jvp[q] = jvp ? jvp[q] : nullptr;
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        any |= a.jvp[q] != nullptr || a.tend[q] != nullptr;
    }
    a.jvp_precip = jvp_precip;
    a.precip = precip;
    a.inv_dz = inv_dz;
    a.n = n;
    a.n_lev = n_lev;
    return any;
}

// What a point keeps between its evaluation and its stores: A = sum − (own flux)·g, value and tangent (final but for the inflow), the fluxes it sends down, g
template <typename FT> struct ColJvpPoint {
    FT Av[CMX_SB2006_JAC_NOUT], Ad[CMX_SB2006_JAC_NOUT];
    FT Fv[4], Fd[4];
    FT g;
};

// The statuses of the J v entry after the NULL checks of the parameter structs: the ladder (cmx_column_products.hpp) with the entry's columns
template <typename FT>
inline int32_t sb2006_column_jvp_status(uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, const FT *const *tangents, FT *const *jvp,
                                        FT *jvp_precip, FT *const *tendencies, FT *precip) {
    const void *given[CMX_SB2006_JAC_NWRT];
    void *outs[2 * CMX_SB2006_JAC_NOUT + 2];
    for (int j = 0; j < CMX_SB2006_JAC_NWRT; ++j) given[j] = tangents ? tangents[j] : nullptr;
    for (int q = 0; q < CMX_SB2006_JAC_NOUT; ++q) {
        outs[q] = jvp ? jvp[q] : nullptr;
        outs[CMX_SB2006_JAC_NOUT + q] = tendencies ? tendencies[q] : nullptr;
    }
    outs[2 * CMX_SB2006_JAC_NOUT] = jvp_precip;
    outs[2 * CMX_SB2006_JAC_NOUT + 1] = precip;
    return column_entry_status(n_col, n_lev, sb2006_column_flags_status(flags), inv_dz, in, nullptr, given, CMX_SB2006_JAC_NWRT, outs, 2 * CMX_SB2006_JAC_NOUT + 2, false);
}

// One evaluation of the scheme on Dual<FT, 1> seeded with the caller's tangent t (0 where the column is NULL), at the level whose 1/Δz is inv_dz.  The NaN
// rule is applied here: a NaN in a state input or in a given tangent of the point → every A of the point; a NaN in an input of the fluxes → the fluxes, value
// and tangent (a NaN tangent reaches them by plain IEEE arithmetic).
template <typename S, typename FT, typename C>
__device__ __forceinline__ void column_jvp_eval(const C &c, const CloudVelConsts<FT> &cv, const FT (&x)[S::NWRT + 1], const FT (&t)[S::NWRT], FT inv_dz, ColJvpPoint<FT> &p) {
    using M = Math<FT>;
    int tnan = 0;
#pragma unroll
    for (int j = 0; j < S::NWRT; ++j) tnan |= (int)(t[j] != t[j]);      // bitwise on purpose: no branch
    const bool poison = products_detail::poison_with<S>(x, (bool)tnan), fpoison = S::flux_poison(x);
    Dual<FT, 1> in[S::NWRT], o[S::NOUT], F[4];
#pragma unroll
    for (int j = 0; j < S::NWRT; ++j) {
        in[j].v = keep(x[j + 1]);
        in[j].d[0] = keep(t[j]);
    }
    S::template eval<FT, 1>(c, cv, keep(x[0]), inv_dz, in, o, F, p.g);
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) {
        p.Av[q] = o[q].v;
        p.Ad[q] = o[q].d[0];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s < S::NFLUX) {      // minus the outflow through the lower face
            const int q = S::flux_out(s);
            p.Av[q] = M::fma(-F[s].v, p.g, p.Av[q]);
            p.Ad[q] = M::fma(-F[s].d[0], p.g, p.Ad[q]);
        }
        p.Fv[s] = S::out(F[s].v, fpoison);
        p.Fd[s] = S::out(F[s].d[0], fpoison);
    }
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) {
        p.Av[q] = S::out(p.Av[q], poison);
        p.Ad[q] = S::out(p.Ad[q], poison);
    }
}

// The inflow through the upper face — the fluxes (upv, upd) the cell above sends down; nothing enters through the model top — and the stores of point i of
// column `col`.  surface: level 0, whose own q_rai flux is the column's precipitation flux.
template <typename S, typename FT>
__device__ __forceinline__ void column_jvp_store(const ColJvpArgs<FT> &a, const ColJvpPoint<FT> &p, const FT (&upv)[4], const FT (&upd)[4], bool top, bool surface,
                                                 int64_t i, int64_t col) {
    using M = Math<FT>;
    FT yv[S::NOUT], yd[S::NOUT];
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) {
        yv[q] = p.Av[q];
        yd[q] = p.Ad[q];
    }
#pragma unroll
    for (int s = 0; s < S::NFLUX; ++s) {
        const int q = S::flux_out(s);
        yv[q] = top ? p.Av[q] : M::fma(upv[s], p.g, p.Av[q]);
        yd[q] = top ? p.Ad[q] : M::fma(upd[s], p.g, p.Ad[q]);
    }
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) {
        if (a.tend[q]) a.tend[q][i] = yv[q];
        if (a.jvp[q]) a.jvp[q][i] = yd[q];
    }
    if (surface) {
        if (a.precip) a.precip[col] = p.Fv[0];
        if (a.jvp_precip) a.jvp_precip[col] = p.Fd[0];
    }
}

// ---- Jᵀ ḡ -----------------------------------------------------------------------------------------------------------------------------------------
// Tangent slot s = pass·K + k as in VjpArgs (cmx_jacobian.hpp).  `cot[q]`: the cotangent column of output q (NULL: structurally absent), `cot_precip`: the
// cotangent of the precipitation flux, one per column (NULL: absent).  `lam[s]`: flux slot s has a multiplier at all (its output's cotangent, or — q_rai — the
// precipitation's, is given).  `nterm`: the terms of a gradient's sum that are present.
template <typename FT, int K> struct ColVjpArgs {
    static constexpr int SLOTS = (CMX_SB2006_JAC_NWRT + K - 1) / K * K;
    const FT *in[CMX_SB2006_JAC_NWRT + 1];
    const FT *cot[CMX_SB2006_JAC_NOUT];
    const FT *cot_precip;
    FT *tend[CMX_SB2006_JAC_NOUT];
    FT *precip;
    FT *grad[SLOTS];
    const FT *inv_dz;
    int64_t n;
    int32_t n_lev;
    int32_t wrt[SLOTS];
    int32_t npass;
    int32_t nterm;
    int32_t lam[4];
    int32_t primal;                   // tend or precip requested
};

// The statuses of the Jᵀḡ entry after the NULL checks of the parameter structs: the ladder (cmx_column_products.hpp) with the entry's columns
template <typename FT>
inline int32_t sb2006_column_vjp_status(uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, const FT *const *cotangents,
                                        const FT *cot_precip, FT *const *grad, FT *const *tendencies, FT *precip) {
    const void *given[CMX_SB2006_JAC_NOUT + 1];
    void *outs[CMX_SB2006_JAC_NOUT + CMX_SB2006_JAC_NWRT + 1];
    for (int q = 0; q < CMX_SB2006_JAC_NOUT; ++q) {
        given[q] = cotangents ? cotangents[q] : nullptr;
        outs[q] = tendencies ? tendencies[q] : nullptr;
    }
    given[CMX_SB2006_JAC_NOUT] = cot_precip;
    for (int j = 0; j < CMX_SB2006_JAC_NWRT; ++j) outs[CMX_SB2006_JAC_NOUT + j] = grad ? grad[j] : nullptr;
    outs[CMX_SB2006_JAC_NOUT + CMX_SB2006_JAC_NWRT] = precip;
    return column_entry_status(n_col, n_lev, sb2006_column_flags_status(flags), inv_dz, in, nullptr, given, CMX_SB2006_JAC_NOUT + 1, outs,
                               CMX_SB2006_JAC_NOUT + CMX_SB2006_JAC_NWRT + 1, false);
}

// An input is wanted if its gradient is not NULL.  False if the call has no output at all.
template <typename FT, int K>
inline bool make_col_vjp_args(ColVjpArgs<FT, K> &a, const FT *const (&in)[CMX_SB2006_JAC_NWRT + 1], const FT *inv_dz, int64_t n, int32_t n_lev,
                              const FT *const *cotangents, const FT *cot_precip, FT *const *grad, FT *const *tendencies, FT *precip) {
    a = ColVjpArgs<FT, K>{};
    for (int j = 0; j < CMX_SB2006_JAC_NWRT + 1; ++j) a.in[j] = in[j];
    bool any = precip != nullptr;
    for (int q = 0; q < CMX_SB2006_JAC_NOUT; ++q) {
        a.cot[q] = cotangents ? cotangents[q] : nullptr;
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        any |= a.tend[q] != nullptr;
    }
    a.primal = any;
    a.cot_precip = cot_precip;
    a.precip = precip;
    a.inv_dz = inv_dz;
    a.n = n;
    a.n_lev = n_lev;
    const int ns = seed_slots<K, CMX_SB2006_JAC_NWRT>(a.wrt, a.npass, [&](int j) { return grad && grad[j]; });
    for (int s = 0; s < ns; ++s) a.grad[s] = grad[a.wrt[s]];
    return any || ns > 0;
}
// the flux slots of the scheme S that have a multiplier, and the count of terms (after make_col_vjp_args, once the instantiation is known)
template <typename S, typename FT, int K> inline void set_col_vjp_terms(ColVjpArgs<FT, K> &a) {
    a.nterm = 0;
    for (int q = 0; q < S::NOUT; ++q) a.nterm += a.cot[q] != nullptr;
    for (int s = 0; s < 4; ++s) {
        a.lam[s] = s < S::NFLUX && (a.cot[S::flux_out(s)] != nullptr || (s == 0 && a.cot_precip != nullptr));
        a.nterm += a.lam[s];
    }
}

// λ of point i = col·n_lev + lev, shared by Jᵀḡ and the parameter gradient (`a`: ColVjpArgs or ColParamVjpArgs): from g_k, g_{k−1}, the cotangents of the
// levels k and k−1, read raw, and p̄.  gnan: p̄ is a NaN.
template <typename S, typename FT, typename A>
__device__ __forceinline__ void column_lambda(const A &a, const FT (&x)[S::NWRT + 1], FT inv_dz, int64_t i, int64_t col, int32_t lev, FT (&lam)[4], int &gnan) {
    using M = Math<FT>;
    using products_detail::ld;
    const bool surface = lev == 0;
    const FT gk = inv_dz * S::inv_rho(x[0]);
    const FT gm = surface ? FT(0) : a.inv_dz[lev - 1] * S::inv_rho(ld(a.in[0], i - 1));
    FT pbar = FT(0);
    if (surface && a.cot_precip) pbar = ld(a.cot_precip, col);
    gnan |= (int)(pbar != pbar);
    for_each_slot<S::NFLUX>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        const FT *const cot = a.cot[S::flux_out(s)];
        FT l = FT(0);
        if (cot) {
            l = -gk * ld(cot, i);
            if (!surface) l = M::fma(gm, ld(cot, i - 1), l);
        }
        if (s == 0 && surface && a.cot_precip) l = l + pbar;
        lam[s] = l;
    });
}

// The primal entry's operations on the value parts of one evaluation, and the stores of the requested primal outputs: A = fma(−F, g, sum), the NaN rule, the
// inflow upv — the flux values of the raw point above (zeros at the top), which the caller gets from the constants it has.
template <typename S, typename FT, typename A, typename D>
__device__ __forceinline__ void column_primal_store(const A &a, const FT (&x)[S::NWRT + 1], const D (&o)[S::NOUT], const D (&F)[4], FT gk, const FT (&upv)[4], bool top,
                                                    bool bad, int64_t i, int64_t col, int32_t lev) {
    using M = Math<FT>;
    FT y[S::NOUT];
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) y[q] = o[q].v;
    for_each_slot<S::NFLUX>([&](auto sc) {
        constexpr int s = decltype(sc)::value, q = S::flux_out(s);
        y[q] = M::fma(-F[s].v, gk, y[q]);
    });
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) y[q] = S::out(y[q], bad);
    for_each_slot<S::NFLUX>([&](auto sc) {
        constexpr int s = decltype(sc)::value, q = S::flux_out(s);
        y[q] = top ? y[q] : M::fma(upv[s], gk, y[q]);
    });
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q)
        if (a.tend[q]) a.tend[q][i] = y[q];
    if (lev == 0 && a.precip) a.precip[col] = S::out(F[0].v, S::flux_poison(x));
}

// Every pass of point i = col·n_lev + lev.  Pointwise: the only neighbour data are ρ_{i−1} and the falling species' ḡ_{i−1}, raw from memory (and, if the
// tendencies are requested, the state of point i+1 for the flux values it sends down).  λ is formed first, then the passes of vjp_point (cmx_jacobian.hpp) run:
// unit seeds, the cotangents read after eval, the sum of a slot as ONE chain of fma seeded with −0 — the point sums with ḡ in output order, then the fluxes with
// λ in slot order — so each gradient comes from its own slot only.  T and q_tot do not enter the fluxes: their slots skip the flux terms.
template <typename S, typename FT, int K, typename C>
__device__ __forceinline__ void column_vjp_point(const C &c, const CloudVelConsts<FT> &cv, const ColVjpArgs<FT, K> &a, const FT (&x)[S::NWRT + 1], int64_t i, int64_t col,
                                                 int32_t lev) {
    using M = Math<FT>;
    using products_detail::ld;
    const bool top = lev == a.n_lev - 1;
    const FT inv_dz = a.inv_dz[lev];
    FT lam[4] = {FT(0), FT(0), FT(0), FT(0)};
    int gnan = 0;
    column_lambda<S, FT>(a, x, inv_dz, i, col, lev, lam, gnan);
    const bool poison = S::poison(x);
    for (int pass = 0; pass < a.npass; ++pass) {
        Dual<FT, K> in[S::NWRT], o[S::NOUT], F[4];
        FT gk;
#pragma unroll
        for (int j = 0; j < S::NWRT; ++j) {
            in[j].v = keep(x[j + 1]);
#pragma unroll
            for (int k = 0; k < K; ++k) in[j].d[k] = a.wrt[pass * K + k] == j ? FT(1) : FT(0);
        }
        S::template eval<FT, K>(c, cv, keep(x[0]), inv_dz, in, o, F, gk);
        FT g[S::NOUT];
        int cnan = gnan;
        const int64_t ic = products_detail::after(i, o[S::NOUT - 1].v);
#pragma unroll
        for (int q = 0; q < S::NOUT; ++q) {
            g[q] = a.cot[q] ? ld(a.cot[q], ic) : FT(0);
            cnan |= (int)(g[q] != g[q]);      // bitwise on purpose: no branch
        }
        const bool bad = (bool)((int)poison | cnan);      // a NaN cotangent of the point poisons its tendencies and gradients too
        if (pass == 0 && a.primal) {
            // the inflow: the primal's flux-only evaluation of the raw point above
            SedFlux<FT> up{FT(0), FT(0), FT(0), FT(0)};
            if (!top) up = S::flux_values(c, cv, ld(a.in[0], i + 1), ld(a.in[3], i + 1), ld(a.in[4], i + 1), ld(a.in[5], i + 1), ld(a.in[6], i + 1));
            const FT upv[4] = {up.q_rai, up.n_rai, up.q_lcl, up.n_lcl};
            column_primal_store<S, FT>(a, x, o, F, gk, upv, top, bad, i, col, lev);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            FT *const out = a.grad[pass * K + k];
            if (!out) continue;
            FT s = a.nterm ? -FT(0) : FT(0);
#pragma unroll
            for (int q = 0; q < S::NOUT; ++q)
                if (a.cot[q]) s = M::fma(g[q], o[q].d[k], s);
            if (a.wrt[pass * K + k] >= CMX_SB2006_JAC_WRT_Q_LCL) {
#pragma unroll
                for (int f = 0; f < S::NFLUX; ++f)
                    if (a.lam[f]) s = M::fma(lam[f], F[f].d[k], s);
            }
            out[i] = S::out(s, bad);
        }
    }
}

}  // namespace cmx
