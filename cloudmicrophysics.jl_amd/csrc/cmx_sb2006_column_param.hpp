// cmx_sb2006_column_param.hpp — what the device entries (cmx_sb2006_column_param.hip) and the host test build (tests/native/column_param_host.cpp,
// CMX_HOST_BUILD) share of the derivatives of the SB2006 COLUMN step with respect to the PARAMETERS (include/cmx.h §(26)): the checks of the directions, the
// constants with their tangents, the argument structs and the bodies of one point.  No HIP in here.
//
// The function is §(25)'s (cmx_sb2006_column_jac.hpp), per column with the state, ρ and inv_dz held fixed:
//     out_k = tend(ρ_k, x_k; θ) + g_k·(F_{k+1}(θ) − F_k(θ)),   g_k = inv_dz[k]·(1/ρ_k⁺),   F_{n_lev} = 0,   precip = F_0[q_rai]
// and the scheme is SbColJac::eval with the roles exchanged, as param_jvp_point (cmx_jacobian.hpp) does for the point function: the state enters as constants
// (structural zeros), SbConsts<Dual<FT, KP>> and CloudVelConsts<Dual<FT, KP>> carry ċ = Dc(θ)[δθ⁽ᵏ⁾] in tangent slot k, folded on the host in exact forward
// mode (make_sb_consts_from with its fall-speed block, make_cloud_vel_consts_from; cmx_param_tangent.hpp).  With Ḟ_k = ∂F_k/∂θ·δθ:
//     J_θ δθ:   ẏ_k = ∂tend/∂θ·δθ + g_k·(Ḟ_{k+1} − Ḟ_k),   ṗ = Ḟ_0[q_rai]
//     gradient: grad[d] = Σ_columns Σ_k ( Σ_o ḡ_{o,k}·(∂tend_o/∂θ·δθ⁽ᵈ⁾)_k + Σ_s λ_k[s]·Ḟ_k[s]⁽ᵈ⁾ ),   λ_k of §(25)
// The VALUE parts and the two fma per falling species are column_jvp_eval's / column_jvp_store's, so requested tendencies and the precipitation flux are the
// primal column entry's bit for bit (no direction on an exponent), and a tangent slot is computed by the same operations whatever KP is and whatever the
// other slots hold.
//
// The Chen-2022 table (vel.chen2022) is held fixed: its constants carry zero tangents, Γ(b_i(ρ) + 1) of the general instantiation is the value
// (cmx_dual.hpp TGammaGeneral), and a direction with a non-zero component there is CMX_ERR_UNSUPPORTED.
//
// KP, the directions per evaluation: tuning numbers (-DCMX_COLPARAM_K_F32=…, -DCMX_COLPARAM_K_F64=…, -DCMX_COLPARAM_K_F64_GEN=…), the widest at which no
// instantiation of either kernel spills a VGPR, executes a scratch instruction or outgrows the 4 KiB kernel-argument segment.  VGPRs over the instantiations
// of a float type, cross-compiled for gfx950 (J_θ δθ kernel | gradient kernel; "sb / chen": SB2006 and fitted Chen-2022 fall speeds, 16 instantiations;
// "gen": general Chen-2022 with run-time Γ, 8):
//     Float32  KP = 1: sb / chen 78–102 | 145–188, gen 93–105 | 201–217      KP = 4: sb / chen 148–185 | 187–263, gen 185–192 | 251–263      none spills: 4
//     Float64  KP = 1: sb / chen 177–268 | 276–384, gen 264–278 | 482–511 (8 spilled)
//              KP = 2: sb / chen 235–294 | 312–431 (1 spilled), gen 278–328 | 510–512 (up to 46 spilled); kernel-argument segment 4168–4176 bytes: 1
// The Float64 gradient kernel of the general Chen-2022 instantiation spills even at KP = 1: it is not built, and the gradient entry returns
// CMX_ERR_UNSUPPORTED for that combination (the J_θ δθ entry serves it).  All of these run at one or two waves per SIMD (512 VGPRs per lane at one wave);
// the LDS halo of the J_θ δθ kernel is 8 KiB (Float32 KP = 1), 20 KiB (KP = 4), 19 KiB (Float64, with the math tables) per workgroup of 256 — never what
// limits the waves.  A column's bits do not depend on KP.
#pragma once
#include <cstdint>
#include <type_traits>

#include "../../include/cmx.h"
#include "cmx_param_tangent.hpp"
#include "cmx_sb2006_column_jac.hpp"

namespace cmx {

#ifndef CMX_COLPARAM_K_F32
#define CMX_COLPARAM_K_F32 4
#endif
#ifndef CMX_COLPARAM_K_F64
#define CMX_COLPARAM_K_F64 1
#endif
#ifndef CMX_COLPARAM_K_F64_GEN
#define CMX_COLPARAM_K_F64_GEN 1
#endif
template <typename FT, int VEL>
constexpr int kColParamK = sizeof(FT) == 4 ? CMX_COLPARAM_K_F32 : (VEL == VEL_CHEN_GEN ? CMX_COLPARAM_K_F64_GEN : CMX_COLPARAM_K_F64);

// The constants of ONE launch: tangent slot k holds ċ of direction d0 + k (an idle slot past ndir: zeros).  Every slot's value parts are the same, and the
// plain fold's, bit for bit.  d_tps, d_vel, d_cloud_vel: NULL is a zero direction; without cloud_vel the cloud constants are zeros and d_cloud_vel is not read.
template <typename FT, int KP, typename WR, typename TH, typename VL, typename ST>
inline void make_column_param_consts(const WR &wr, const TH &tps, const VL &vel, const ST *cloud_vel, const WR *d_wr, const TH *d_tps, const VL *d_vel,
                                     const ST *d_cloud_vel, int d0, int ndir, SbConsts<Dual<FT, KP>> &cd, CloudVelConsts<Dual<FT, KP>> &cvd) {
    cd = SbConsts<Dual<FT, KP>>{};
    cvd = CloudVelConsts<Dual<FT, KP>>{};
    for (int k = 0; k < KP; ++k) {
        const bool live = d0 + k < ndir;
        const ParamReader<WR> P{wr, live ? d_wr + d0 + k : nullptr};
        const SbConsts<ParamTan> ct = make_sb_consts_from<FT, ParamTan>(wr, tps, &vel, (double)Math<FT>::eps_1m(), P,
                                                                        ParamReader<TH>{tps, live && d_tps ? d_tps + d0 + k : nullptr},
                                                                        ParamReader<VL>{vel, live && d_vel ? d_vel + d0 + k : nullptr});
        pack_param_consts<KP>(ct, k, cd);
        if (cloud_vel) {
            const CloudVelConsts<ParamTan> cvt = make_cloud_vel_consts_from<FT, ParamTan>(
                wr.seifert_beheng.pdf_c, *cloud_vel, P, ParamReader<ST>{*cloud_vel, live && d_cloud_vel ? d_cloud_vel + d0 + k : nullptr});
            pack_param_consts<KP>(cvt, k, cvd);
        }
    }
}
// next to the constants the kernel-argument segment holds the column tables, the geometry and the reduction's arguments: at most 320 bytes at KP ≤ 4
static_assert(sizeof(SbConsts<Dual<float, CMX_COLPARAM_K_F32>>) + sizeof(CloudVelConsts<Dual<float, CMX_COLPARAM_K_F32>>) + 320 <= 4096 &&
                  sizeof(SbConsts<Dual<double, CMX_COLPARAM_K_F64>>) + sizeof(CloudVelConsts<Dual<double, CMX_COLPARAM_K_F64>>) + 320 <= 4096,
              "CMX_COLPARAM_K_*: the constants with their tangents must fit the 4 KiB kernel-argument segment");

// The checks of the directions and the instantiation choice, after the entry's own argument checks and in this order: 1 ≤ ndir ≤ CMX_PARAM_MAX_DIRS and the
// table; finite components (CMX_ERR_BAD_ARG); a non-zero component on the Chen-2022 table (CMX_ERR_UNSUPPORTED, whatever the flags); the limiters and the
// fall-speed parameters of the primal entry.  The integer-exponent instantiation runs only if the primal entry would select it AND no direction moves
// acnv.b, accr.c or self.d.  d_cloud_vel is not looked at without cloud_vel.  Returns f(SbColJac<…>{}).
template <typename FT, typename WR, typename TH, typename VL, typename ST, typename F>
inline int32_t with_sb2006_column_param(const WR &wr, const TH &tps, const VL &vel, const ST *cloud_vel, uint32_t flags, int32_t ndir, const WR *d_wr, const TH *d_tps,
                                        const VL *d_vel, const ST *d_cloud_vel, F &&f) {
    if (ndir < 1 || ndir > CMX_PARAM_MAX_DIRS || !d_wr) return CMX_ERR_BAD_ARG;
    bool exponents = false, chen = false;
    for (int d = 0; d < ndir; ++d) {
        if (!all_finite<FT>(d_wr[d]) || (d_tps && !all_finite<FT>(d_tps[d])) || (d_vel && !all_finite<FT>(d_vel[d])) ||
            (cloud_vel && d_cloud_vel && !all_finite<FT>(d_cloud_vel[d])))
            return CMX_ERR_BAD_ARG;
        const auto &sb = d_wr[d].seifert_beheng;
        exponents |= sb.acnv.b != 0 || sb.accr.c != 0 || sb.self.d != 0;
        if (d_vel) {
            const FT *p = reinterpret_cast<const FT *>(&d_vel[d].chen2022);
            for (size_t i = 0; i < sizeof(d_vel[d].chen2022) / sizeof(FT); ++i) chen |= p[i] != FT(0);
        }
    }
    if (chen) return CMX_ERR_UNSUPPORTED;
    const bool limited = flags & CMX_SB2006_LIMITED, sbv = flags & CMX_VEL_SB2006;
    if (limited && !sb_limiters_ok(wr)) return CMX_ERR_BAD_ARG;
    if (sbv && !sb_rain_vel_ok(vel, limited)) return CMX_ERR_BAD_ARG;
    const int velk = sbv ? VEL_SB : chen_vel_kind<FT>(vel.chen2022);
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG,
                       [&](auto L, auto V, auto CL, auto I) -> int32_t {
                           return f(SbColJac<decltype(L)::value, decltype(V)::value, decltype(CL)::value, decltype(I)::value>{});
                       },
                       flag(limited), one_of<VEL_SB, VEL_CHEN, VEL_CHEN_GEN>(velk), flag(cloud_vel != nullptr), flag(sb_integer_exponents(wr) && !exponents));
}

// The statuses of the two entries after the NULL checks of the parameter structs and before with_sb2006_column_param: the ladder (cmx_column_products.hpp)
// with the entry's columns.  The seven columns and inv_dz are compared with the outputs even without a point.
template <typename FT>
inline int32_t sb2006_column_param_jvp_status(uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, int32_t ndir, const void *d_wr,
                                              FT *const *jvp, FT *const *jvp_precip, FT *const *tendencies, FT *precip) {
    void *outs[CMX_PARAM_MAX_DIRS * (CMX_SB2006_JAC_NOUT + 1) + CMX_SB2006_JAC_NOUT + 1];
    int nouts = 0;
    const int nd = ndir < 0 ? 0 : (ndir > CMX_PARAM_MAX_DIRS ? CMX_PARAM_MAX_DIRS : ndir);
    for (int q = 0; q < nd * CMX_SB2006_JAC_NOUT && jvp; ++q) outs[nouts++] = jvp[q];
    for (int d = 0; d < nd && jvp_precip; ++d) outs[nouts++] = jvp_precip[d];
    for (int q = 0; q < CMX_SB2006_JAC_NOUT && tendencies; ++q) outs[nouts++] = tendencies[q];
    outs[nouts++] = precip;
    const ColumnDirs dirs{ndir, d_wr};
    return column_entry_status(n_col, n_lev, sb2006_column_flags_status(flags), inv_dz, in, &dirs, nullptr, 0, outs, nouts, false);
}
// grad and workspace are required
template <typename FT>
inline int32_t sb2006_column_param_vjp_status(uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, const FT *const *cotangents,
                                              const FT *cot_precip, int32_t ndir, const void *d_wr, double *grad, double *workspace, FT *const *tendencies, FT *precip) {
    const void *given[CMX_SB2006_JAC_NOUT + 1];
    void *outs[CMX_SB2006_JAC_NOUT + 3];
    for (int q = 0; q < CMX_SB2006_JAC_NOUT; ++q) {
        given[q] = cotangents ? cotangents[q] : nullptr;
        outs[q] = tendencies ? tendencies[q] : nullptr;
    }
    given[CMX_SB2006_JAC_NOUT] = cot_precip;
    outs[CMX_SB2006_JAC_NOUT] = precip;
    outs[CMX_SB2006_JAC_NOUT + 1] = grad;
    outs[CMX_SB2006_JAC_NOUT + 2] = workspace;
    const ColumnDirs dirs{ndir, d_wr};
    return column_entry_status(n_col, n_lev, sb2006_column_flags_status(flags), inv_dz, in, &dirs, given, CMX_SB2006_JAC_NOUT + 1, outs, CMX_SB2006_JAC_NOUT + 3, true);
}

// ---- one evaluation ---------------------------------------------------------------------------------------------------------------------------------
// What a point keeps between its evaluation and its stores: ColJvpPoint with KP tangents, the struct that the halo shell shares between the schemes
template <typename FT, int KP> using ColParamPoint = ColumnPoint<FT, KP>;

// column_jvp_eval with the KP tangents of the constants.  The NaN rule is the primal's: a NaN in a state input → every A of the point; a NaN in an input of
// the fluxes → the fluxes, value and tangents.
template <typename S, typename FT, int KP, typename CD, typename CVD>
__device__ __forceinline__ void column_param_eval(const CD &cd, const CVD &cvd, const FT (&x)[S::NWRT + 1], FT inv_dz, ColumnPoint<FT, KP> &p) {
    using M = Math<FT>;
    const bool poison = S::poison(x), fpoison = S::flux_poison(x);
    Dual<FT, KP> in[S::NWRT], o[S::NOUT], F[4];
#pragma unroll
    for (int j = 0; j < S::NWRT; ++j) in[j] = Dual<FT, KP>(x[j + 1]);
    S::template eval<FT, KP>(cd, cvd, x[0], inv_dz, in, o, F, p.g);
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) {
        p.Av[q] = o[q].v;
#pragma unroll
        for (int k = 0; k < KP; ++k) p.Ad[k][q] = o[q].d[k];
    }
    for_each_slot<4>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        if constexpr (s < S::NFLUX) {      // minus the outflow through the lower face
            constexpr int q = S::flux_out(s);
            p.Av[q] = M::fma(-F[s].v, p.g, p.Av[q]);
#pragma unroll
            for (int k = 0; k < KP; ++k) p.Ad[k][q] = M::fma(-F[s].d[k], p.g, p.Ad[k][q]);
        }
        p.Fv[s] = S::out(F[s].v, fpoison);
#pragma unroll
        for (int k = 0; k < KP; ++k) p.Fd[k][s] = S::out(F[s].d[k], fpoison);
    });
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) {
        p.Av[q] = S::out(p.Av[q], poison);
#pragma unroll
        for (int k = 0; k < KP; ++k) p.Ad[k][q] = S::out(p.Ad[k][q], poison);
    }
}

// ---- J_θ δθ -----------------------------------------------------------------------------------------------------------------------------------------
// `jvp[k][q]`: the column of direction slot k, output q; `jvp_precip[k]`: one value per column; `tend`, `precip`: the primal.  All NULL-able.
template <typename FT, int KP> struct ColParamJvpArgs {
    const FT *in[CMX_SB2006_JAC_NWRT + 1];      // rho, then the other inputs
    FT *tend[CMX_SB2006_JAC_NOUT];
    FT *precip;
    FT *jvp[KP][CMX_SB2006_JAC_NOUT];
    FT *jvp_precip[KP];
    const FT *inv_dz;
    int64_t n;                                   // n_col · n_lev
    int32_t n_lev;
};

// The arguments of the launch of the directions d0 … d0 + KP − 1; the primal outputs go with the first launch.  False if the launch has no output at all.
template <typename FT, int KP>
inline bool make_column_param_jvp_args(ColParamJvpArgs<FT, KP> &a, const FT *const (&in)[CMX_SB2006_JAC_NWRT + 1], const FT *inv_dz, int64_t n, int32_t n_lev, int d0,
                                       int ndir, FT *const *jvp, FT *const *jvp_precip, FT *const *tendencies, FT *precip) {
    a = ColParamJvpArgs<FT, KP>{};
    for (int j = 0; j < CMX_SB2006_JAC_NWRT + 1; ++j) a.in[j] = in[j];
    bool wanted = false;
    for (int q = 0; q < CMX_SB2006_JAC_NOUT; ++q) wanted |= (a.tend[q] = d0 == 0 && tendencies ? tendencies[q] : nullptr) != nullptr;
    wanted |= (a.precip = d0 == 0 ? precip : nullptr) != nullptr;
    for (int k = 0; k < KP && d0 + k < ndir; ++k) {
        for (int q = 0; q < CMX_SB2006_JAC_NOUT && jvp; ++q) wanted |= (a.jvp[k][q] = jvp[(d0 + k) * CMX_SB2006_JAC_NOUT + q]) != nullptr;
        if (jvp_precip) wanted |= (a.jvp_precip[k] = jvp_precip[d0 + k]) != nullptr;
    }
    a.inv_dz = inv_dz;
    a.n = n;
    a.n_lev = n_lev;
    return wanted;
}

// The inflow through the upper face — the fluxes (upv, upd) the cell above sends down; nothing enters through the model top — and the stores of point i of
// column `col` (column_jvp_store with KP tangents).
template <typename S, typename FT, int KP>
__device__ __forceinline__ void column_param_jvp_store(const ColParamJvpArgs<FT, KP> &a, const ColumnPoint<FT, KP> &p, const FT (&upv)[4], const FT (&upd)[KP][4],
                                                       bool top, bool surface, int64_t i, int64_t col) {
    using M = Math<FT>;
    FT yv[S::NOUT];
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) yv[q] = p.Av[q];
    for_each_slot<S::NFLUX>([&](auto sc) {
        constexpr int s = decltype(sc)::value, q = S::flux_out(s);
        yv[q] = top ? p.Av[q] : M::fma(upv[s], p.g, p.Av[q]);
    });
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q)
        if (a.tend[q]) a.tend[q][i] = yv[q];
    if (surface && a.precip) a.precip[col] = p.Fv[0];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        FT yd[S::NOUT];
#pragma unroll
        for (int q = 0; q < S::NOUT; ++q) yd[q] = p.Ad[k][q];
        for_each_slot<S::NFLUX>([&](auto sc) {
            constexpr int s = decltype(sc)::value, q = S::flux_out(s);
            yd[q] = top ? p.Ad[k][q] : M::fma(upd[k][s], p.g, p.Ad[k][q]);
        });
#pragma unroll
        for (int q = 0; q < S::NOUT; ++q)
            if (a.jvp[k][q]) a.jvp[k][q][i] = yd[q];
        if (surface && a.jvp_precip[k]) a.jvp_precip[k][col] = p.Fd[k][0];
    }
}

// ---- the gradient -----------------------------------------------------------------------------------------------------------------------------------
// `cot[q]`: the cotangent column of output q (NULL: absent), `cot_precip`: one per column (NULL: absent); `lam[s]`, `nterm`: as in ColVjpArgs.
template <typename FT> struct ColParamVjpArgs {
    const FT *in[CMX_SB2006_JAC_NWRT + 1];
    const FT *cot[CMX_SB2006_JAC_NOUT];
    const FT *cot_precip;
    FT *tend[CMX_SB2006_JAC_NOUT];
    FT *precip;
    const FT *inv_dz;
    int64_t n;
    int32_t n_lev;
    int32_t nterm;
    int32_t lam[4];
    int32_t primal;                   // tend or precip requested (the first launch only)
};

template <typename S, typename FT>
inline void make_column_param_vjp_args(ColParamVjpArgs<FT> &a, const FT *const (&in)[CMX_SB2006_JAC_NWRT + 1], const FT *inv_dz, int64_t n, int32_t n_lev,
                                       const FT *const *cotangents, const FT *cot_precip, bool first, FT *const *tendencies, FT *precip) {
    a = ColParamVjpArgs<FT>{};
    for (int j = 0; j < CMX_SB2006_JAC_NWRT + 1; ++j) a.in[j] = in[j];
    bool any = first && precip != nullptr;
    for (int q = 0; q < CMX_SB2006_JAC_NOUT; ++q) {
        a.cot[q] = cotangents ? cotangents[q] : nullptr;
        a.tend[q] = first && tendencies ? tendencies[q] : nullptr;
        any |= a.tend[q] != nullptr;
        a.nterm += a.cot[q] != nullptr;
    }
    a.primal = any;
    a.cot_precip = cot_precip;
    a.precip = first ? precip : nullptr;
    a.inv_dz = inv_dz;
    a.n = n;
    a.n_lev = n_lev;
    for (int s = 0; s < 4; ++s) {
        a.lam[s] = s < S::NFLUX && (a.cot[S::flux_out(s)] != nullptr || (s == 0 && cot_precip != nullptr));
        a.nterm += a.lam[s];
    }
}

// the VALUE of the fluxes of the raw point above, from the constants that hold duals: the operations of sed_fluxes_of_point on the value parts (a requested
// primal output of the gradient entry needs them; the tangents are dead)
template <typename S, typename FT, int KP, typename CD, typename CVD>
__device__ __forceinline__ void column_param_flux_values(const CD &cd, const CVD &cvd, FT rho, FT q_lcl, FT n_lcl, FT q_rai, FT n_rai, FT (&up)[4]) {
    using D = Dual<FT, KP>;
    using MD = Math<D>;
    const FT eps = Math<FT>::eps();
    const D r_ = D(max0(rho)), ql = D(max0(q_lcl)), nl = D(max0(n_lcl)), qr = D(max0(q_rai)), nr = D(max0(n_rai));
    const D rs_rho = MD::rsqrt(r_);
    const D N_rai = r_ * nr;
    const D L_rai = r_ * MD::max(qr, eps);
    const SbRainPsd<D> psd = sb2006_rain_psd<D, S::limited>(cd, L_rai, MD::max(N_rai, eps));
    D vt_n, vt_m;
    sb2006_rain_velocity<D, S::limited, S::vel>(cd, r_, rs_rho, psd.l2_lam, N_rai < eps, qr < eps, vt_n, vt_m);
    const SedFlux<D> f = sed_fluxes<D, S::cloud>(cvd, r_, ql, nl, qr, nr, vt_n, vt_m);
    const bool bad = any_nan(rho, q_lcl, n_lcl, q_rai, n_rai);
    up[0] = S::out(f.q_rai.v, bad);
    up[1] = S::out(f.n_rai.v, bad);
    up[2] = S::out(f.q_lcl.v, bad);
    up[3] = S::out(f.n_lcl.v, bad);
}

// One point of the gradient: pointwise plus ρ and ḡ of the level below, as column_vjp_point.  λ first, then ONE evaluation for the KP directions; per slot
// the sum is one chain of fma seeded with −0 (no term at all: +0) — the point sums with ḡ in output order, then the fluxes with λ in slot order — widened to
// double and added to the lane's accumulator.  A NaN in the state, in a cotangent of the point or in what λ reads makes the sum NaN.
template <typename S, typename FT, int KP, typename CD, typename CVD>
__device__ __forceinline__ void column_param_vjp_point(const CD &cd, const CVD &cvd, const ColParamVjpArgs<FT> &a, const FT (&x)[S::NWRT + 1], int64_t i, int64_t col,
                                                       int32_t lev, double (&acc)[KP]) {
    using M = Math<FT>;
    using products_detail::ld;
    const bool top = lev == a.n_lev - 1;
    const FT inv_dz = a.inv_dz[lev];
    FT lam[4] = {FT(0), FT(0), FT(0), FT(0)};
    int gnan = 0;
    column_lambda<S, FT>(a, x, inv_dz, i, col, lev, lam, gnan);
    const bool poison = S::poison(x);
    Dual<FT, KP> in[S::NWRT], o[S::NOUT], F[4];
    FT gk;
#pragma unroll
    for (int j = 0; j < S::NWRT; ++j) in[j] = Dual<FT, KP>(x[j + 1]);
    S::template eval<FT, KP>(cd, cvd, x[0], inv_dz, in, o, F, gk);
    FT g[S::NOUT];
    int cnan = gnan;
    const int64_t ic = products_detail::after(i, o[S::NOUT - 1].v);
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) {
        g[q] = a.cot[q] ? ld(a.cot[q], ic) : FT(0);
        cnan |= (int)(g[q] != g[q]);      // bitwise on purpose: no branch
    }
    const bool bad = (bool)((int)poison | cnan);
    if (a.primal) {
        // the inflow: the flux values of the raw point above, from the constants that hold duals
        FT upv[4] = {FT(0), FT(0), FT(0), FT(0)};
        if (!top)
            column_param_flux_values<S, FT, KP>(cd, cvd, ld(a.in[0], i + 1), ld(a.in[3], i + 1), ld(a.in[4], i + 1), ld(a.in[5], i + 1), ld(a.in[6], i + 1), upv);
        column_primal_store<S, FT>(a, x, o, F, gk, upv, top, bad, i, col, lev);
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        FT s = a.nterm ? -FT(0) : FT(0);
#pragma unroll
        for (int q = 0; q < S::NOUT; ++q)
            if (a.cot[q]) s = M::fma(g[q], o[q].d[k], s);
#pragma unroll
        for (int f = 0; f < S::NFLUX; ++f)
            if (a.lam[f]) s = M::fma(lam[f], F[f].d[k], s);
        acc[k] += (double)S::out(s, bad);
    }
}

}  // namespace cmx
