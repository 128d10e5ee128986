// cmx_mp1m_column_jac.hpp — what the device entries (cmx_mp1m_column_products.hip) and the host test build (tests/native/column_products_1m_host.cpp,
// CMX_HOST_BUILD) share of the products J v and Jᵀḡ with the Jacobian of the 1-moment COLUMN step (include/cmx.h §(27)): the scheme Mp1mColJac — the point
// evaluation of Mp1mJac (mp1m_point + mp1m_aggregate, cmx_mp1m.hpp) and the four sedimentation fluxes of cmx_mp1m_vel.hpp on the dual value type
// (cmx_dual.hpp), and g — its set-up from the parameter structs, the argument structs, and the bodies of one point.  No HIP in here.  The shape is that of
// cmx_sb2006_column_jac.hpp; what differs: four falling species, always, TWO surface fluxes (rain and snow), and a flux F[s] that depends on its own species
// q_s (and ρ) only.
//
// The function that is differentiated, per column (level 0 lowest, x_k = (T, q_tot, q_lcl, q_icl, q_rai, q_sno)_k; ρ and inv_dz are held fixed):
//     out_k = tend(ρ_k, x_k) + g_k·(F_{k+1} − F_k),   g_k = inv_dz[k]·rcp(ρ_k⁺),   F_{n_lev} = 0,   precip_rai = F_0[q_rai],   precip_sno = F_0[q_sno]
// F_k[s] = ρ⁺χ⁺w_s for s = q_lcl, q_icl, q_rai, q_sno: the fluxes of mp1m_sed_fluxes.  With Ḟ_k = (∂F_k/∂x_k)·v_k:
//     J v:   ẏ_k = J_pt(x_k)·v_k + g_k·(Ḟ_{k+1} − Ḟ_k),   ṗ_rai = Ḟ_0[q_rai],   ṗ_sno = Ḟ_0[q_sno]
//     Jᵀḡ:   x̄_k = J_pt(x_k)ᵀ·ḡ_k + (∂F_k/∂x_k)ᵀ·λ_k,   λ_k[s] = −g_k·ḡ_k[s] + [k>0]·g_{k−1}·ḡ_{k−1}[s] + [k=0]·p̄_s   (p̄_s: rain and snow only)
// ∂F_k[s]/∂x_k has ONE non-zero entry, ∂F_k[s]/∂q_s: the gradient of q_s takes the one term λ_k[s]·∂F_k[s]/∂q_s, those of T and q_tot none.
// The VALUE parts are formed by the operations of the primal kernel (cmx_mp1m_column_body.inc) in its order — t through the NaN rule, A = fma(−F, g, t),
// then fma(top ? 0 : F_above, g, A) — so requested tendencies and the precipitation fluxes are that entry's (nsub = 0), bit for bit; the tangents take the
// same two fma.
#pragma once
#include <cstdint>
#include <type_traits>

#include "../../include/cmx.h"
#include "cmx_column_products.hpp"
#include "cmx_dispatch.hpp"
#include "cmx_jacobian.hpp"
#include "cmx_mp1m_jacobian.hpp"
#include "cmx_mp1m_vel.hpp"

namespace cmx {

// Tangents per evaluation of the point function in the Jᵀḡ kernel: tuning numbers (-DCMX_COL1M_VJP_K_F32=…, -DCMX_COL1M_VJP_K_F64=…,
// -DCMX_COL1M_VJP_K_F64_GEN=…).  VGPRs, cross-compiled for gfx950, of the run-time-flags | default-options instantiation:
//     Float32   fitted Γ    K = 1: 140 | 188    K = 2: 167 | 208    K = 3: 194 | 220    K = 4: 228 | 258    K = 6: 288 | 334
//               general Γ   K = 1: 154 | 202    K = 2: 181 | 223    K = 3: 201 | 249    K = 4: 235 | 280    K = 6: 289 | 340     none spills
//     Float64   fitted Γ    K = 1: 316 | 406    K = 2: 350 | 434    K = 3: 370 | 462    K = 4: 434 | 512, 18 spilled    K = 6: 512 | 512, 60 | 217 spilled
//               general Γ   K = 1: 388 | 480    K = 2: 420 | 506    K = 3: 450 | 512, 46 spilled    K = 4: 512 | 512, 0 | 150 spilled
// (5 serves the six inputs in two passes like 3 and 4 and was not compiled.)  Float64: the widest K at which no instantiation spills a VGPR — 3, and 2 with
// the general Γ; every Float64 width runs one wave per SIMD, so the fewest passes win.  Float32: 6 is the widest that does not spill, but it runs ONE wave
// per SIMD (more than 256 VGPRs) where 3 runs two, and measured slower on an MI355X — 1e6 points of 64 levels, all six gradients, default parameters, the
// two builds alternating in one session (tools/time_column_products_1m.py): K = 6 0.185–0.187 ms, K = 3 0.123–0.124 ms; at 1e7 points 1.78–1.79 against
// 1.14 ms.  3 is shipped (4 has 258–280 VGPRs in the default-options instantiation: one wave, and two passes like 3).
// No instantiation at the chosen K has a private segment; up to 22 (Float32) and 205 (Float64) SGPRs are parked in VGPR lanes, as in the pointwise
// vjp_kernel of the scheme.  A gradient's bits do not depend on K.
// J v carries the caller's one tangent: Float32 102 | 144 VGPRs, Float64 228–248 | 318–334; the two Float64 default-options instantiations keep the
// 100-byte frame of 8–10 spilled SGPRs (VGPR lanes, no scratch instruction) that the pointwise jvp_kernel<Mp1mJac<default>, double> has: it is the point
// function's — reading the kernel's twelve output pointers through the kernel-argument segment after the point (tried) leaves it as it is.
#ifndef CMX_COL1M_VJP_K_F32
#define CMX_COL1M_VJP_K_F32 3
#endif
#ifndef CMX_COL1M_VJP_K_F64
#define CMX_COL1M_VJP_K_F64 3
#endif
#ifndef CMX_COL1M_VJP_K_F64_GEN
#define CMX_COL1M_VJP_K_F64_GEN 2
#endif
template <typename FT, bool GENERAL> constexpr int kCol1mVjpK = sizeof(FT) == 4 ? CMX_COL1M_VJP_K_F32 : (GENERAL ? CMX_COL1M_VJP_K_F64_GEN : CMX_COL1M_VJP_K_F64);

// The constants of the column scheme: ONE by-value kernel argument, the first, read through the kernel-argument pointer in both float types as in the primal
// column kernel (cmx_mp1m_column.hip Mp1mColKernArgs); `c` comes first, so a reference to it is what mp1m_point's own front_consts would form.
template <typename FT> struct Mp1mColJacConsts {
    Mp1mConsts<FT> c;
    Vel1mConsts<FT> vc;
};

// The column scheme of point x = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno): Mp1mJac's four tendencies, the four fluxes the point sends down, and g.  Flux
// slot s: 0 q_lcl, 1 q_icl, 2 q_rai, 3 q_sno (SedFlux4); the output whose tendency the flux enters is s, the one input it depends on flux_wrt(s).
template <uint32_t FLAGS, bool GENERAL> struct Mp1mColJac {
    using P = Mp1mJac<FLAGS>;
    static constexpr int NOUT = CMX_MP1M_JAC_NOUT, NWRT = CMX_MP1M_JAC_NWRT, NFLUX = 4;
    static constexpr int RAI = 2, SNO = 3;                                  // the flux slots with a surface output
    static constexpr uint32_t flags = FLAGS;
    static constexpr bool general = GENERAL;
    static constexpr int flux_wrt(int s) { return CMX_MP1M_JAC_WRT_Q_LCL + s; }
    static_assert(CMX_MP1M_JAC_DQ_LCL_DT == 0 && CMX_MP1M_JAC_DQ_SNO_DT == 3 && CMX_MP1M_JAC_WRT_Q_SNO == CMX_MP1M_JAC_WRT_Q_LCL + 3, "flux slot s ↔ output s ↔ input Q_LCL + s");
    // The poison rule of the 1-moment entries per point (Mp1mJac), and that of the flux of species s (mp1m_sed_fluxes): a NaN in ρ or q_s — in Float64 also
    // ρ ≤ 0 — reaches the cell below through it
    template <typename FT> static __device__ __forceinline__ bool poison(const FT (&x)[NWRT + 1]) { return P::poison(x); }
    template <typename FT> static __device__ __forceinline__ bool flux_poison(const FT (&x)[NWRT + 1], int s) {
        return (bool)((int)any_nan(x[0], x[1 + flux_wrt(s)]) | (int)bad_density(x[0]));
    }
    template <typename FT> static __device__ __forceinline__ FT out(FT v, bool bad) { return bad ? Math<FT>::nan() : v; }
    // g as the primal kernel forms it: 1/(ρ_k Δz_k) with the library's reciprocal of the clamped density
    template <typename FT> static __device__ __forceinline__ FT g_of(FT rho, FT inv_dz) { return inv_dz * Math<FT>::rcp(max0(rho)); }
    // in: the six differentiated inputs in the order of cmx_mp1m_jac_wrt; o: the point's tendencies (before the NaN rule), F: the fluxes (before theirs).
    // a0: the kernel's constants argument.  The fluxes run the fall speeds of cmx_mp1m_vel.hpp species by species on the clamped duals, in the order and with
    // the phase boundaries of mp1m_sed_fluxes; Γ of the Chen rain curve sees ρ only — a constant — and so carries no tangent in either instantiation.
    template <typename FT, int K, typename CA>
    static __device__ __forceinline__ void eval(const CA &a0, FT rho, const Dual<FT, K> (&in)[NWRT], Dual<FT, K> (&o)[NOUT], Dual<FT, K> (&F)[4]) {
        using D = Dual<FT, K>;
        const auto &a = front_consts<FT, true>(a0);
        const Mp1mSrc<D> p = mp1m_point<D, FLAGS>(a.c, D(rho), in[CMX_MP1M_JAC_WRT_T], in[CMX_MP1M_JAC_WRT_Q_TOT], in[CMX_MP1M_JAC_WRT_Q_LCL],
                                                  in[CMX_MP1M_JAC_WRT_Q_ICL], in[CMX_MP1M_JAC_WRT_Q_RAI], in[CMX_MP1M_JAC_WRT_Q_SNO]);
        mp1m_aggregate<D>(p, o[CMX_MP1M_JAC_DQ_LCL_DT], o[CMX_MP1M_JAC_DQ_ICL_DT], o[CMX_MP1M_JAC_DQ_RAI_DT], o[CMX_MP1M_JAC_DQ_SNO_DT]);
        const auto &vc = consts_after(a, o[NOUT - 1]).vc;
        const D r_ = D(max0(rho));
        const D ql = max0(in[CMX_MP1M_JAC_WRT_Q_LCL]), qi = max0(in[CMX_MP1M_JAC_WRT_Q_ICL]), qr = max0(in[CMX_MP1M_JAC_WRT_Q_RAI]), qs = max0(in[CMX_MP1M_JAC_WRT_Q_SNO]);
        F[0] = (r_ * ql) * vel_lcl_stokes<D>(vc, r_, ql);
        const auto &v1 = consts_after(vc, F[0]);
        const D l2_rho = log2_floored(r_);
        F[1] = (r_ * qi) * vel_icl_chen<D>(v1, r_, r_, qi, l2_rho);
        const auto &v2 = consts_after(v1, F[1]);
        F[2] = (r_ * qr) * vel_rain_chen<D, GENERAL>(v2, r_, vel_l2_li_rain<D>(v2, r_, qr), qr, GENERAL ? log2_floored(keep(r_)) : l2_rho);
        const auto &v3 = consts_after(v2, F[2]);
        F[3] = (r_ * qs) * vel_snow_chen<D, false>(v3, r_, vel_l2_li_snow<D>(v3, r_, qs), qs, l2_rho);
    }
    // the VALUE of the fluxes of a raw point, NaN rule applied: the primal's flux-only evaluation (the cell above, when Jᵀḡ is asked for the tendencies)
    template <typename FT, typename CA>
    static __device__ __forceinline__ SedFlux4<FT> flux_values(const CA &a0, FT rho, FT q_lcl, FT q_icl, FT q_rai, FT q_sno) {
        return mp1m_sed_fluxes<FT, GENERAL, false>(front_consts<FT, true>(a0).vc, rho, q_lcl, q_icl, q_rai, q_sno);
    }
};

// The statuses of the primal entry's flag checks, in its order — both snow-shape bits, then the option bits — and this entry's own: a single snow-shape bit is
// not built (the oracle's column step has no shaped snow to difference against)
inline int32_t mp1m_column_jac_flags_status(uint32_t flags) {
    const uint32_t shape_bits = flags & (CMX_1M_SED_SNOW_OBLATE | CMX_1M_SED_SNOW_PROLATE);
    if (shape_bits == (CMX_1M_SED_SNOW_OBLATE | CMX_1M_SED_SNOW_PROLATE)) return CMX_ERR_BAD_ARG;
    if (const int32_t st = check_flags_1m(flags & ~shape_bits)) return st;
    return shape_bits ? CMX_ERR_UNSUPPORTED : CMX_OK;
}

// The set-up the device entries and the host mirror share after the flag, count and column checks: the constants as the primal entry folds them, and the
// instantiation it selects for the same parameter structs (flags_1m; fitted or general Γ of the Chen rain table).  Returns f(a, Mp1mColJac<…>{}).
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI, typename F>
inline int32_t with_mp1m_column_jac(const MP &mp, const TH &tps, const ST &stokes, const CH &chen_rain, const CI &chen_ice, uint32_t flags, F &&f) {
    Mp1mColJacConsts<FT> a{};
    a.c = make_mp1m_consts<FT>(mp, tps, flags, (double)Math<FT>::eps_1m());
    bool general = false;
    a.vc = make_vel1m_consts<FT>(mp, &chen_rain, &general);
    add_sedimentation_consts<FT>(a.vc, mp, &stokes, &chen_ice);
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG,
                       [&](auto FL, auto GG) -> int32_t { return f(a, Mp1mColJac<decltype(FL)::value, decltype(GG)::value>{}); },
                       flags_1m(flags, a.c), flag(general));
}

// ---- J v ------------------------------------------------------------------------------------------------------------------------------------------
// `tan[j]`: the tangent column of differentiated input j (NULL: zero).  `jvp[q]`, `tend[q]`: n values each; `jvp_precip[r]`, `precip[r]` (r = 0 rain,
// 1 snow): one per column.  All NULL-able.
template <typename FT> struct Col1mJvpArgs {
    const FT *in[CMX_MP1M_JAC_NWRT + 1];      // rho, then the differentiated inputs
    const FT *tan[CMX_MP1M_JAC_NWRT];
    FT *jvp[CMX_MP1M_JAC_NOUT];
    FT *tend[CMX_MP1M_JAC_NOUT];
    FT *jvp_precip[2], *precip[2];
    const FT *inv_dz;
    int64_t n;                                 // n_col · n_lev
    int32_t n_lev;
};

// False if the call has no output at all
template <typename FT>
inline bool make_col1m_jvp_args(Col1mJvpArgs<FT> &a, const FT *const (&in)[CMX_MP1M_JAC_NWRT + 1], const FT *inv_dz, int64_t n, int32_t n_lev, const FT *const *tangents,
                                FT *const *jvp, FT *jvp_precip_rai, FT *jvp_precip_sno, FT *const *tendencies, FT *precip_rai, FT *precip_sno) {
    a = Col1mJvpArgs<FT>{};
    for (int j = 0; j < CMX_MP1M_JAC_NWRT + 1; ++j) a.in[j] = in[j];
    for (int j = 0; j < CMX_MP1M_JAC_NWRT; ++j) a.tan[j] = tangents ? tangents[j] : nullptr;
    bool any = jvp_precip_rai || jvp_precip_sno || precip_rai || precip_sno;
    for (int q = 0; q < CMX_MP1M_JAC_NOUT; ++q) {
        a.jvp[q] = jvp ? jvp[q] : nullptr;
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        any |= a.jvp[q] != nullptr || a.tend[q] != nullptr;
    }
    a.jvp_precip[0] = jvp_precip_rai;
    a.jvp_precip[1] = jvp_precip_sno;
    a.precip[0] = precip_rai;
    a.precip[1] = precip_sno;
    a.inv_dz = inv_dz;
    a.n = n;
    a.n_lev = n_lev;
    return any;
}

// What a point keeps between its evaluation and its stores: A = t − (own flux)·g, value and tangent (final but for the inflow), the fluxes it sends down, g
template <typename FT> struct Col1mJvpPoint {
    FT Av[CMX_MP1M_JAC_NOUT], Ad[CMX_MP1M_JAC_NOUT];
    FT Fv[4], Fd[4];
    FT g;
};

// The statuses of the J v entry after the NULL checks of the parameter structs: the ladder (cmx_column_products.hpp) with the entry's columns
template <typename FT>
inline int32_t mp1m_column_jvp_status(uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, const FT *const *tangents, FT *const *jvp,
                                      FT *jvp_precip_rai, FT *jvp_precip_sno, FT *const *tendencies, FT *precip_rai, FT *precip_sno) {
    const void *given[CMX_MP1M_JAC_NWRT];
    void *outs[2 * CMX_MP1M_JAC_NOUT + 4];
    for (int j = 0; j < CMX_MP1M_JAC_NWRT; ++j) given[j] = tangents ? tangents[j] : nullptr;
    for (int q = 0; q < CMX_MP1M_JAC_NOUT; ++q) {
        outs[q] = jvp ? jvp[q] : nullptr;
        outs[CMX_MP1M_JAC_NOUT + q] = tendencies ? tendencies[q] : nullptr;
    }
    outs[2 * CMX_MP1M_JAC_NOUT] = jvp_precip_rai;
    outs[2 * CMX_MP1M_JAC_NOUT + 1] = jvp_precip_sno;
    outs[2 * CMX_MP1M_JAC_NOUT + 2] = precip_rai;
    outs[2 * CMX_MP1M_JAC_NOUT + 3] = precip_sno;
    return column_entry_status(n_col, n_lev, mp1m_column_jac_flags_status(flags), inv_dz, in, nullptr, given, CMX_MP1M_JAC_NWRT, outs, 2 * CMX_MP1M_JAC_NOUT + 4, false);
}

// One evaluation of the scheme on Dual<FT, 1> seeded with the caller's tangent t (0 where the column is NULL), at the level whose 1/Δz is inv_dz.  The NaN
// rule is applied here, where the primal applies it: a NaN in a state input or in a given tangent of the point → every tendency of the point, value and
// tangent, BEFORE the own flux is subtracted; a NaN in ρ or q_s → the flux of species s, value and tangent (a NaN tangent reaches it by plain IEEE arithmetic).
template <typename S, typename FT, typename CA>
__device__ __forceinline__ void column1m_jvp_eval(const CA &a0, const FT (&x)[S::NWRT + 1], const FT (&t)[S::NWRT], FT inv_dz, Col1mJvpPoint<FT> &p) {
    using M = Math<FT>;
    int tnan = 0;
#pragma unroll
    for (int j = 0; j < S::NWRT; ++j) tnan |= (int)(t[j] != t[j]);      // bitwise on purpose: no branch
    const bool poison = products_detail::poison_with<S>(x, (bool)tnan);
    Dual<FT, 1> in[S::NWRT], o[S::NOUT], F[4];
#pragma unroll
    for (int j = 0; j < S::NWRT; ++j) {
        in[j].v = keep(x[j + 1]);
        in[j].d[0] = keep(t[j]);
    }
    S::template eval<FT, 1>(a0, keep(x[0]), in, o, F);
    p.g = S::g_of(x[0], inv_dz);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const bool fpoison = S::flux_poison(x, s);
        p.Fv[s] = S::out(F[s].v, fpoison);
        p.Fd[s] = S::out(F[s].d[0], fpoison);
        // minus the outflow through the lower face
        p.Av[s] = M::fma(-p.Fv[s], p.g, S::out(o[s].v, poison));
        p.Ad[s] = M::fma(-p.Fd[s], p.g, S::out(o[s].d[0], poison));
    }
}

// The inflow through the upper face — the fluxes (upv, upd) the cell above sends down; nothing enters through the model top: a zero flux, multiplied out as in
// the primal — and the stores of point i of column `col`.  surface: level 0, whose own rain and snow fluxes are the column's precipitation fluxes.
template <typename S, typename FT>
__device__ __forceinline__ void column1m_jvp_store(const Col1mJvpArgs<FT> &a, const Col1mJvpPoint<FT> &p, const FT (&upv)[4], const FT (&upd)[4], bool top, bool surface,
                                                   int64_t i, int64_t col) {
    using M = Math<FT>;
#pragma unroll
    for (int s = 0; s < S::NOUT; ++s) {
        const FT yv = M::fma(top ? FT(0) : upv[s], p.g, p.Av[s]);
        const FT yd = M::fma(top ? FT(0) : upd[s], p.g, p.Ad[s]);
        if (a.tend[s]) a.tend[s][i] = yv;
        if (a.jvp[s]) a.jvp[s][i] = yd;
    }
    if (surface) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (a.precip[r]) a.precip[r][col] = p.Fv[S::RAI + r];
            if (a.jvp_precip[r]) a.jvp_precip[r][col] = p.Fd[S::RAI + r];
        }
    }
}

// ---- Jᵀ ḡ -----------------------------------------------------------------------------------------------------------------------------------------
// Tangent slot s = pass·K + k as in VjpArgs (cmx_jacobian.hpp).  `cot[q]`: the cotangent column of output q (NULL: structurally absent), `cot_precip[r]`: the
// cotangent of the rain / snow precipitation flux, one per column (NULL: absent).  `lam[s]`: flux slot s has a multiplier at all (its output's cotangent, or
// — rain, snow — the precipitation's, is given).  `ncot`: the non-NULL members of cot.
template <typename FT, int K> struct Col1mVjpArgs {
    static constexpr int SLOTS = (CMX_MP1M_JAC_NWRT + K - 1) / K * K;
    const FT *in[CMX_MP1M_JAC_NWRT + 1];
    const FT *cot[CMX_MP1M_JAC_NOUT];
    const FT *cot_precip[2];
    FT *tend[CMX_MP1M_JAC_NOUT];
    FT *precip[2];
    FT *grad[SLOTS];
    const FT *inv_dz;
    int64_t n;
    int32_t n_lev;
    int32_t wrt[SLOTS];
    int32_t npass;
    int32_t ncot;
    int32_t lam[4];
    int32_t primal;                   // tend or precip requested
};

// The statuses of the Jᵀḡ entry after the NULL checks of the parameter structs: the ladder (cmx_column_products.hpp) with the entry's columns
template <typename FT>
inline int32_t mp1m_column_vjp_status(uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, const FT *const *cotangents,
                                      const FT *cot_precip_rai, const FT *cot_precip_sno, FT *const *grad, FT *const *tendencies, FT *precip_rai, FT *precip_sno) {
    const void *given[CMX_MP1M_JAC_NOUT + 2];
    void *outs[CMX_MP1M_JAC_NOUT + CMX_MP1M_JAC_NWRT + 2];
    for (int q = 0; q < CMX_MP1M_JAC_NOUT; ++q) {
        given[q] = cotangents ? cotangents[q] : nullptr;
        outs[q] = tendencies ? tendencies[q] : nullptr;
    }
    given[CMX_MP1M_JAC_NOUT] = cot_precip_rai;
    given[CMX_MP1M_JAC_NOUT + 1] = cot_precip_sno;
    for (int j = 0; j < CMX_MP1M_JAC_NWRT; ++j) outs[CMX_MP1M_JAC_NOUT + j] = grad ? grad[j] : nullptr;
    outs[CMX_MP1M_JAC_NOUT + CMX_MP1M_JAC_NWRT] = precip_rai;
    outs[CMX_MP1M_JAC_NOUT + CMX_MP1M_JAC_NWRT + 1] = precip_sno;
    return column_entry_status(n_col, n_lev, mp1m_column_jac_flags_status(flags), inv_dz, in, nullptr, given, CMX_MP1M_JAC_NOUT + 2, outs,
                               CMX_MP1M_JAC_NOUT + CMX_MP1M_JAC_NWRT + 2, false);
}

// An input is wanted if its gradient is not NULL.  False if the call has no output at all.
template <typename FT, int K>
inline bool make_col1m_vjp_args(Col1mVjpArgs<FT, K> &a, const FT *const (&in)[CMX_MP1M_JAC_NWRT + 1], const FT *inv_dz, int64_t n, int32_t n_lev, const FT *const *cotangents,
                                const FT *cot_precip_rai, const FT *cot_precip_sno, FT *const *grad, FT *const *tendencies, FT *precip_rai, FT *precip_sno) {
    a = Col1mVjpArgs<FT, K>{};
    for (int j = 0; j < CMX_MP1M_JAC_NWRT + 1; ++j) a.in[j] = in[j];
    bool any = precip_rai != nullptr || precip_sno != nullptr;
    for (int q = 0; q < CMX_MP1M_JAC_NOUT; ++q) {
        a.cot[q] = cotangents ? cotangents[q] : nullptr;
        a.ncot += a.cot[q] != nullptr;
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        any |= a.tend[q] != nullptr;
    }
    a.primal = any;
    a.cot_precip[0] = cot_precip_rai;
    a.cot_precip[1] = cot_precip_sno;
    a.precip[0] = precip_rai;
    a.precip[1] = precip_sno;
    a.inv_dz = inv_dz;
    a.n = n;
    a.n_lev = n_lev;
    for (int s = 0; s < 4; ++s) a.lam[s] = a.cot[s] != nullptr || (s >= 2 && a.cot_precip[s - 2] != nullptr);
    const int ns = seed_slots<K, CMX_MP1M_JAC_NWRT>(a.wrt, a.npass, [&](int j) { return grad && grad[j]; });
    for (int s = 0; s < ns; ++s) a.grad[s] = grad[a.wrt[s]];
    return any || ns > 0;
}

// λ of point i = col·n_lev + lev, shared by Jᵀḡ and the parameter gradient (`a`: Col1mVjpArgs or Col1mParamVjpArgs): from g_k, g_{k−1}, the cotangents of
// the levels k and k−1, read raw, and p̄ of rain and snow.  gnan: a p̄ is a NaN.
template <typename S, typename FT, typename A>
__device__ __forceinline__ void column1m_lambda(const A &a, const FT (&x)[S::NWRT + 1], FT gk, int64_t i, int64_t col, int32_t lev, FT (&lam)[4], int &gnan) {
    using M = Math<FT>;
    using products_detail::ld;
    const bool surface = lev == 0;
    const FT gm = surface ? FT(0) : S::g_of(ld(a.in[0], i - 1), a.inv_dz[lev - 1]);
    for_each_slot<4>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        const FT *const cot = a.cot[s];
        FT l = FT(0);
        if (cot) {
            l = -gk * ld(cot, i);
            if (!surface) l = M::fma(gm, ld(cot, i - 1), l);
        }
        if constexpr (s >= 2) {
            if (surface && a.cot_precip[s - 2]) {
                const FT pbar = ld(a.cot_precip[s - 2], col);
                gnan |= (int)(pbar != pbar);
                l = l + pbar;
            }
        }
        lam[s] = l;
    });
}

// Every pass of point i = col·n_lev + lev.  Pointwise: the only neighbour data are ρ_{i−1} and the cotangents ḡ_{i−1}, raw from memory (and, if the
// tendencies are requested, the state of point i+1 for the flux values it sends down).  λ is formed first, then the passes of vjp_point (cmx_jacobian.hpp) run:
// unit seeds, the cotangents read after eval, the sum of a slot as ONE chain of fma seeded with −0 (a slot with no term at all: +0) — the tendencies with ḡ in
// output order, then, in the slot of q_s, the one flux term λ[s]·∂F[s]/∂q_s — so each gradient comes from its own slot only.
template <typename S, typename FT, int K, typename CA>
__device__ __forceinline__ void column1m_vjp_point(const CA &a0, const Col1mVjpArgs<FT, K> &a, const FT (&x)[S::NWRT + 1], int64_t i, int64_t col, int32_t lev) {
    using M = Math<FT>;
    using products_detail::ld;
    const bool top = lev == a.n_lev - 1;
    const FT gk = S::g_of(x[0], a.inv_dz[lev]);
    FT lam[4] = {FT(0), FT(0), FT(0), FT(0)};
    int gnan = 0;
    column1m_lambda<S, FT>(a, x, gk, i, col, lev, lam, gnan);
    const bool poison = S::poison(x);
    for (int pass = 0; pass < a.npass; ++pass) {
        Dual<FT, K> in[S::NWRT], o[S::NOUT], F[4];
#pragma unroll
        for (int j = 0; j < S::NWRT; ++j) {
            in[j].v = keep(x[j + 1]);
#pragma unroll
            for (int k = 0; k < K; ++k) in[j].d[k] = a.wrt[pass * K + k] == j ? FT(1) : FT(0);
        }
        S::template eval<FT, K>(a0, keep(x[0]), in, o, F);
        FT g[S::NOUT];
        int cnan = gnan;
        const int64_t ic = products_detail::after(i, F[3].v);
#pragma unroll
        for (int q = 0; q < S::NOUT; ++q) {
            g[q] = a.cot[q] ? ld(a.cot[q], ic) : FT(0);
            cnan |= (int)(g[q] != g[q]);      // bitwise on purpose: no branch
        }
        const bool bad = (bool)((int)poison | cnan);      // a NaN cotangent of the point poisons its tendencies and gradients too
        if (pass == 0 && a.primal) {
            // the primal entry's operations: t through the NaN rule, A = fma(−F, g, t), the inflow from the flux-only evaluation of the raw point above.
            // (Not shared with column1m_param_vjp_point, which has the same block in its own text: written once, as a function over the flux slots, the
            // sign bit of the NaN that a point with a NaN tendency AND a NaN own flux stores came out differently from this loop's.)
            SedFlux4<FT> up{{FT(0), FT(0), FT(0), FT(0)}};
            if (!top) up = S::flux_values(a0, ld(a.in[0], i + 1), ld(a.in[3], i + 1), ld(a.in[4], i + 1), ld(a.in[5], i + 1), ld(a.in[6], i + 1));
#pragma unroll
            for (int s = 0; s < S::NOUT; ++s) {
                const FT Fv = S::out(F[s].v, S::flux_poison(x, s));
                const FT A = M::fma(-Fv, gk, S::out(o[s].v, bad));
                if (a.tend[s]) a.tend[s][i] = M::fma(top ? FT(0) : up.f[s], gk, A);
                if (s >= 2 && lev == 0 && a.precip[s - 2]) a.precip[s - 2][col] = Fv;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            FT *const out = a.grad[pass * K + k];
            if (!out) continue;
            const int32_t j = a.wrt[pass * K + k];
            const int32_t f = j - S::flux_wrt(0);      // the flux slot of this input, if it is a falling species
            const bool fterm = f >= 0 && a.lam[f >= 0 ? f : 0];
            FT s = (a.ncot || fterm) ? -FT(0) : FT(0);
#pragma unroll
            for (int q = 0; q < S::NOUT; ++q)
                if (a.cot[q]) s = M::fma(g[q], o[q].d[k], s);
            if (fterm) {
                FT l = lam[0], Fd = F[0].d[k];
#pragma unroll
                for (int t = 1; t < 4; ++t) {      // selects over constant indices: no register array is indexed by a run-time value
                    l = f == t ? lam[t] : l;
                    Fd = f == t ? F[t].d[k] : Fd;
                }
                s = M::fma(l, Fd, s);
            }
            out[i] = S::out(s, bad);
        }
    }
}

}  // namespace cmx
