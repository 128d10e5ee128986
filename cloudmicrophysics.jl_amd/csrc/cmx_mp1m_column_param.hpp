// cmx_mp1m_column_param.hpp — what the device entries (cmx_mp1m_column_param.hip) and the host test build (tests/native/column_param_1m_host.cpp,
// CMX_HOST_BUILD) share of the derivatives of the 1-moment COLUMN step with respect to the PARAMETERS (include/cmx.h §(28)): the checks of the directions, the
// constants with their tangents, the argument structs and the bodies of one point.  No HIP in here.  The shape is that of cmx_sb2006_column_param.hpp.
//
// The function is §(27)'s (cmx_mp1m_column_jac.hpp), per column with the state, ρ and inv_dz held fixed:
//     out_k = tend(ρ_k, x_k; θ) + g_k·(F_{k+1}(θ) − F_k(θ)),   g_k = inv_dz[k]·rcp(ρ_k⁺),   F_{n_lev} = 0,   precip_rai = F_0[q_rai],   precip_sno = F_0[q_sno]
// and the scheme is Mp1mColJac::eval with the roles exchanged: the state enters as constants (structural zeros), Mp1mConsts<Dual<FT, KP>> and the velocity
// constants carry ċ = Dc(θ)[δθ⁽ᵏ⁾] in tangent slot k, folded on the host in exact forward mode (make_mp1m_consts_from, make_vel1m_consts_from,
// add_sedimentation_consts_from; cmx_param_tangent.hpp), and the fall-speed functions of cmx_mp1m_vel.hpp run on duals unchanged.  With Ḟ_k = ∂F_k/∂θ·δθ:
//     J_θ δθ:   ẏ_k = ∂tend/∂θ·δθ + g_k·(Ḟ_{k+1} − Ḟ_k),   ṗ_rai = Ḟ_0[q_rai],   ṗ_sno = Ḟ_0[q_sno]
//     gradient: grad[d] = Σ_columns Σ_k ( Σ_o ḡ_{o,k}·(∂tend_o/∂θ·δθ⁽ᵈ⁾)_k + Σ_s λ_k[s]·Ḟ_k[s]⁽ᵈ⁾ ),   λ_k of §(27)
// The VALUE parts and the two fma per falling species are column1m_jvp_eval's / column1m_jvp_store's, so requested tendencies and the precipitation fluxes are
// the primal column entry's bit for bit (no direction on an exponent), and a tangent slot is computed by the same operations whatever KP is and whatever the
// other slots hold.
//
// What carries no tangent: ε and log2 ε, log2 1000, and b[3], b_ρ of the Chen-2022 rain table with the Γ(b − b_ρ ρ + 4)/3! they feed (the fitted polynomials
// ChenGamma<FT>, or the run-time Γ on the value: cmx_dual.hpp TGammaGeneral).  They are plain FT members of the constants (Vel1mTanConsts), structural
// zeros in the arithmetic; a direction with a non-zero component on b or b_ρ is CMX_ERR_UNSUPPORTED.
//
// With inv_dz ≡ 0 the four jvp rows are those of cmx_mp1m_param_jvp_* under == wherever Ḟ of the point and of the point above is finite: the two fma per
// species then add ∓0·Ḟ.  (Float32: an absent species has log2 0 = −Inf in its fall speed, whose tangent is discarded by the gate q > ε — Ḟ is 0 there.)
//
// KP, the directions per evaluation: tuning numbers (-DCMX_COLPARAM1M_K_F32=…, -DCMX_COLPARAM1M_K_F64=…, -DCMX_COLPARAM1M_K_F64_GEN=…), the widest at which no
// instantiation of either kernel spills a VGPR, executes a scratch instruction or outgrows the 4 KiB kernel-argument segment.  VGPRs over the four
// instantiations of a float type (run-time flags | default options, each with the fitted and the general Γ), cross-compiled for gfx950 (J_θ δθ kernel |
// gradient kernel; kernel-argument bytes):
//     Float32  KP = 1:  92–101 | 127–178 (1344 | 1392 B)    KP = 2: 121–123 | 168–199 (1920 B)    KP = 3: 148–152 | 202–228 (2488 | 2440 B)
//              KP = 4: 175–183 | 232–252 (3064 | 2968 B); fitted Γ 175–176 | 232–244, general Γ 175–183 | 249–252                          none spills: 4
//     Float64  KP = 1: fitted Γ 228–256 | 264–346, general Γ 233–282 | 384–474 (2848 | 2896 B)
//              KP = 2: fitted Γ 262–284 | 316–368, general Γ 266–308 | 426–498 (3944 B)                                                     none spills: 2
//              KP = 3: the constants alone are 131 duals of 32 bytes, 4192 bytes: they outgrow the segment
// No instantiation executes a scratch instruction; private segments of 0–132 bytes are the frames of SGPRs parked in VGPR lanes.  Float32 at KP = 4 stays
// at or below 256 VGPRs (two waves per SIMD), so no timing decides; every Float64 width runs one wave per SIMD, so the fewest passes win.  The Float64
// gradient kernel of the general-Γ instantiation does not spill, so every combination is served by both entries.  The LDS halo of the J_θ δθ kernel is
// 8–20 KiB (Float32), 19–27 KiB (Float64, with the math tables) per workgroup of 256 — never what limits the waves.  A column's bits do not depend on KP.
#pragma once
#include <cstdint>
#include <type_traits>

#include "../../include/cmx.h"
#include "cmx_mp1m_column_jac.hpp"
#include "cmx_param_tangent.hpp"

namespace cmx {

#ifndef CMX_COLPARAM1M_K_F32
#define CMX_COLPARAM1M_K_F32 4
#endif
#ifndef CMX_COLPARAM1M_K_F64
#define CMX_COLPARAM1M_K_F64 2
#endif
#ifndef CMX_COLPARAM1M_K_F64_GEN
#define CMX_COLPARAM1M_K_F64_GEN 2
#endif
template <typename FT, bool GENERAL>
constexpr int kCol1mParamK = sizeof(FT) == 4 ? CMX_COLPARAM1M_K_F32 : (GENERAL ? CMX_COLPARAM1M_K_F64_GEN : CMX_COLPARAM1M_K_F64);

// The constants of the four column fall speeds (Stokes cloud liquid, Chen-2022 small ice, rain, large ice) the way the parameter derivatives hold them: the
// members of Vel1mConsts the fall speeds read, under the same names.  Vel1mTanPart: what carries a tangent, scalars of ONE type (pack_param_consts);
// Vel1mTanConsts adds what carries none as plain S.
template <typename T> struct Vel1mTanPart {
    T lam_a_rai, lam_b_rai, lam_floor_rai, lam_a_sno, lam_b_sno, lam_floor_sno, sno_l2_mu, sno_nu;
    T ch_rho0_l2e, ch_a[3], ch_a3_pow, ch_c1000[3];
    T st_pref, st_rho_w, st_D3;
    T ci_D3, ci_A, ci_B, ci_C, ci_E, ci_F, ci_c2;
    T sn_A, sn_a1, sn_b1, sn_a2, sn_H, sn_b2, sn_c2;
};
template <typename T, typename S> struct Vel1mTanConsts : Vel1mTanPart<T> {
    S eps_1m, l2_eps, l2_1000, ch_b[3], ch_b_rho;
    ChenGamma<S> chg;
};

// ONE by-value kernel argument, the first: the point function's constants and the fall speeds', tangent slot k of every dual member = ċ of direction d0 + k
template <typename FT, int KP> struct Col1mParamConsts {
    Mp1mConsts<Dual<FT, KP>> c;
    Vel1mTanConsts<Dual<FT, KP>, FT> vc;
};
// next to the constants the kernel-argument segment holds the column tables, the geometry and the reduction's arguments: at most 400 bytes at KP ≤ 4
static_assert(sizeof(Col1mParamConsts<float, CMX_COLPARAM1M_K_F32>) + 400 <= 4096 && sizeof(Col1mParamConsts<double, CMX_COLPARAM1M_K_F64>) + 400 <= 4096 &&
                  sizeof(Col1mParamConsts<double, CMX_COLPARAM1M_K_F64_GEN>) + 400 <= 4096,
              "CMX_COLPARAM1M_K_*: the constants with their tangents must fit the 4 KiB kernel-argument segment");

// The fold of ONE direction on ParamTan (NULL tables: zero): the point function's constants and the fall speeds'.  The value parts are the plain folds' —
// make_mp1m_consts, make_vel1m_consts, add_sedimentation_consts — in every bit.  *general: the rain table needs the run-time Γ.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
inline void make_col1m_tangent_consts(const MP &mp, const TH &tps, const ST &stokes, const CH &chen_rain, const CI &chen_ice, uint32_t flags, const MP *d_mp,
                                      const TH *d_tps, const ST *d_stokes, const CH *d_chen_rain, const CI *d_chen_ice, Mp1mConsts<ParamTan> &ct,
                                      Vel1mTanConsts<ParamTan, FT> &vt, bool *general = nullptr) {
    const ParamReader<MP> P{mp, d_mp};
    ct = make_mp1m_tangent_consts<FT>(mp, tps, flags, d_mp, d_tps);
    vt = Vel1mTanConsts<ParamTan, FT>{};
    make_vel1m_consts_from<FT, ParamTan>(vt, mp, &chen_rain, general, P, ParamReader<CH>{chen_rain, d_chen_rain});
    add_sedimentation_consts_from<FT>(vt, mp, &stokes, &chen_ice, (uint32_t)CMX_SNOW_SHAPE_ASPR, P, ParamReader<ST>{stokes, d_stokes},
                                      ParamReader<CI>{chen_ice, d_chen_ice});
}

// The constants of ONE launch: tangent slot k holds ċ of direction d0 + k (an idle slot past ndir: zeros).  Every slot's value parts are the same.
template <typename FT, int KP, typename MP, typename TH, typename ST, typename CH, typename CI>
inline void make_col1m_param_consts(const MP &mp, const TH &tps, const ST &stokes, const CH &chen_rain, const CI &chen_ice, uint32_t flags, const MP *d_mp,
                                    const TH *d_tps, const ST *d_stokes, const CH *d_chen_rain, const CI *d_chen_ice, int d0, int ndir, Col1mParamConsts<FT, KP> &a) {
    a = Col1mParamConsts<FT, KP>{};
    a.c.flags = flags;
    for (int k = 0; k < KP; ++k) {
        const bool live = d0 + k < ndir;
        Mp1mConsts<ParamTan> ct;
        Vel1mTanConsts<ParamTan, FT> vt;
        make_col1m_tangent_consts<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, live ? d_mp + d0 + k : nullptr, live && d_tps ? d_tps + d0 + k : nullptr,
                                      live && d_stokes ? d_stokes + d0 + k : nullptr, live && d_chen_rain ? d_chen_rain + d0 + k : nullptr,
                                      live && d_chen_ice ? d_chen_ice + d0 + k : nullptr, ct, vt);
        pack_param_members<KP>(ct, &ct.eps_1m, k, a.c, &a.c.eps_1m);
        pack_param_consts<KP>(static_cast<const Vel1mTanPart<ParamTan> &>(vt), k, static_cast<Vel1mTanPart<Dual<FT, KP>> &>(a.vc));
        a.vc.eps_1m = vt.eps_1m; a.vc.l2_eps = vt.l2_eps; a.vc.l2_1000 = vt.l2_1000; a.vc.ch_b_rho = vt.ch_b_rho; a.vc.chg = vt.chg;
        for (int i = 0; i < 3; ++i) a.vc.ch_b[i] = vt.ch_b[i];
    }
}

// The column scheme on constants that hold duals.  x = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), raw; o: the point's tendencies (before the NaN rule),
// F: the fluxes (before theirs), in the order and with the operations of Mp1mColJac::eval.  The clamped state enters the fluxes as constants.
template <uint32_t FLAGS, bool GENERAL> struct Mp1mColParam : Mp1mColJac<FLAGS, GENERAL> {
    using B = Mp1mColJac<FLAGS, GENERAL>;
    template <typename FT, int K, typename VD> static __device__ __forceinline__ void fluxes(const VD &vc, FT rho, FT q_lcl, FT q_icl, FT q_rai, FT q_sno, Dual<FT, K> (&F)[4]) {
        using D = Dual<FT, K>;
        const D r_ = D(max0(rho)), ql = D(max0(q_lcl)), qi = D(max0(q_icl)), qr = D(max0(q_rai)), qs = D(max0(q_sno));
        F[0] = (r_ * ql) * vel_lcl_stokes<D>(vc, r_, ql);
        const D l2_rho = log2_floored(r_);
        F[1] = (r_ * qi) * vel_icl_chen<D>(vc, r_, r_, qi, l2_rho);
        F[2] = (r_ * qr) * vel_rain_chen<D, GENERAL>(vc, r_, vel_l2_li_rain<D>(vc, r_, qr), qr, GENERAL ? log2_floored(keep(r_)) : l2_rho);
        F[3] = (r_ * qs) * vel_snow_chen<D, false>(vc, r_, vel_l2_li_snow<D>(vc, r_, qs), qs, l2_rho);
    }
    template <typename FT, int K, typename CA>
    static __device__ __forceinline__ void eval(const CA &a, const FT (&x)[B::NWRT + 1], Dual<FT, K> (&o)[B::NOUT], Dual<FT, K> (&F)[4]) {
        using D = Dual<FT, K>;
        const Mp1mSrc<D> p = mp1m_point<D, FLAGS>(a.c, D(x[0]), D(x[1 + CMX_MP1M_JAC_WRT_T]), D(x[1 + CMX_MP1M_JAC_WRT_Q_TOT]), D(x[1 + CMX_MP1M_JAC_WRT_Q_LCL]),
                                                  D(x[1 + CMX_MP1M_JAC_WRT_Q_ICL]), D(x[1 + CMX_MP1M_JAC_WRT_Q_RAI]), D(x[1 + CMX_MP1M_JAC_WRT_Q_SNO]));
        mp1m_aggregate<D>(p, o[CMX_MP1M_JAC_DQ_LCL_DT], o[CMX_MP1M_JAC_DQ_ICL_DT], o[CMX_MP1M_JAC_DQ_RAI_DT], o[CMX_MP1M_JAC_DQ_SNO_DT]);
        fluxes<FT, K>(a.vc, x[0], x[3], x[4], x[5], x[6], F);
    }
};

// The checks of the directions and the instantiation choice, after the entry's own argument checks and in this order: 1 ≤ ndir ≤ CMX_PARAM_MAX_DIRS and the
// table; finite components (CMX_ERR_BAD_ARG); a non-zero component on b or b_ρ of the Chen-2022 rain table (CMX_ERR_UNSUPPORTED, whatever the flags).  The
// default-options instantiation runs only if the primal entry would select it AND no direction moves one of the nine slope-parameter exponents it holds at
// compile time (with_mp1m_param); fitted or general Γ as the primal entry chooses.  Returns f(Mp1mColParam<…>{}).
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI, typename F>
inline int32_t with_mp1m_column_param(const MP &mp, const TH &tps, const ST &stokes, const CH &chen_rain, const CI &chen_ice, uint32_t flags, int32_t ndir,
                                      const MP *d_mp, const TH *d_tps, const ST *d_stokes, const CH *d_chen_rain, const CI *d_chen_ice, F &&f) {
    if (ndir < 1 || ndir > CMX_PARAM_MAX_DIRS || !d_mp) return CMX_ERR_BAD_ARG;
    for (int d = 0; d < ndir; ++d)
        if (!all_finite<FT>(d_mp[d]) || (d_tps && !all_finite<FT>(d_tps[d])) || (d_stokes && !all_finite<FT>(d_stokes[d])) ||
            (d_chen_rain && !all_finite<FT>(d_chen_rain[d])) || (d_chen_ice && !all_finite<FT>(d_chen_ice[d])))
            return CMX_ERR_BAD_ARG;
    bool exponents = false, gamma = false;
    for (int d = 0; d < ndir; ++d) {
        const Mp1mConsts<ParamTan> t = make_mp1m_tangent_consts<FT>(mp, tps, flags, d_mp + d, d_tps ? d_tps + d : nullptr);
        for (const ParamTan &e : {t.vt_e_rai, t.acc_e_rai, t.sink_e, t.rs_dp1_rai, t.ven_e_rai, t.vt_e_sno, t.acc_e_sno, t.rs_dp1_sno, t.ven_e_sno}) exponents |= e.d != 0;
        if (d_chen_rain) {
            const CH &r = d_chen_rain[d];
            gamma |= r.b[0] != FT(0) || r.b[1] != FT(0) || r.b[2] != FT(0) || r.b_rho != FT(0);
        }
    }
    if (gamma) return CMX_ERR_UNSUPPORTED;
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(mp, tps, flags, (double)Math<FT>::eps_1m());
    bool general = false;
    (void)make_vel1m_consts<FT>(mp, &chen_rain, &general);
    const bool fast = flags == CMX_1M_DEFAULT_OPTIONS && mp1m_default_exponents(c) && !exponents;
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG,
                       [&](auto FL, auto GG) -> int32_t { return f(Mp1mColParam<decltype(FL)::value, decltype(GG)::value>{}); },
                       one_of<kDefaultFlags, kRuntimeFlags>(fast ? kDefaultFlags : kRuntimeFlags), flag(general));
}

// The statuses of the two entries after the NULL checks of the parameter structs and before with_mp1m_column_param: the ladder (cmx_column_products.hpp)
// with the entry's columns.  The columns and inv_dz are looked at only when there is a point.
template <typename FT>
inline int32_t mp1m_column_param_jvp_status(uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, int32_t ndir, const void *d_mp,
                                            FT *const *jvp, FT *const *jvp_precip_rai, FT *const *jvp_precip_sno, FT *const *tendencies, FT *precip_rai, FT *precip_sno) {
    void *outs[CMX_PARAM_MAX_DIRS * (CMX_MP1M_JAC_NOUT + 2) + CMX_MP1M_JAC_NOUT + 2];
    int nouts = 0;
    const int nd = ndir < 0 ? 0 : (ndir > CMX_PARAM_MAX_DIRS ? CMX_PARAM_MAX_DIRS : ndir);
    for (int q = 0; q < nd * CMX_MP1M_JAC_NOUT && jvp; ++q) outs[nouts++] = jvp[q];
    for (int d = 0; d < nd && jvp_precip_rai; ++d) outs[nouts++] = jvp_precip_rai[d];
    for (int d = 0; d < nd && jvp_precip_sno; ++d) outs[nouts++] = jvp_precip_sno[d];
    for (int q = 0; q < CMX_MP1M_JAC_NOUT && tendencies; ++q) outs[nouts++] = tendencies[q];
    outs[nouts++] = precip_rai;
    outs[nouts++] = precip_sno;
    const ColumnDirs dirs{ndir, d_mp};
    const bool points = n_col > 0;
    return column_entry_status(n_col, n_lev, mp1m_column_jac_flags_status(flags), points ? inv_dz : nullptr, points ? in : nullptr, &dirs, nullptr, 0, outs, nouts, false);
}
// grad and workspace are required
template <typename FT>
inline int32_t mp1m_column_param_vjp_status(uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, const FT *const *cotangents,
                                            const FT *cot_precip_rai, const FT *cot_precip_sno, int32_t ndir, const void *d_mp, double *grad, double *workspace,
                                            FT *const *tendencies, FT *precip_rai, FT *precip_sno) {
    const void *given[CMX_MP1M_JAC_NOUT + 2];
    void *outs[CMX_MP1M_JAC_NOUT + 4];
    for (int q = 0; q < CMX_MP1M_JAC_NOUT; ++q) {
        given[q] = cotangents ? cotangents[q] : nullptr;
        outs[q] = tendencies ? tendencies[q] : nullptr;
    }
    given[CMX_MP1M_JAC_NOUT] = cot_precip_rai;
    given[CMX_MP1M_JAC_NOUT + 1] = cot_precip_sno;
    outs[CMX_MP1M_JAC_NOUT] = precip_rai;
    outs[CMX_MP1M_JAC_NOUT + 1] = precip_sno;
    outs[CMX_MP1M_JAC_NOUT + 2] = grad;
    outs[CMX_MP1M_JAC_NOUT + 3] = workspace;
    const ColumnDirs dirs{ndir, d_mp};
    const bool points = n_col > 0;
    return column_entry_status(n_col, n_lev, mp1m_column_jac_flags_status(flags), points ? inv_dz : nullptr, points ? in : nullptr, &dirs, given, CMX_MP1M_JAC_NOUT + 2,
                               outs, CMX_MP1M_JAC_NOUT + 4, true);
}

// ---- one evaluation ---------------------------------------------------------------------------------------------------------------------------------
// What a point keeps between its evaluation and its stores: Col1mJvpPoint with KP tangents, the struct that the halo shell shares between the schemes
template <typename FT, int KP> using Col1mParamPoint = ColumnPoint<FT, KP>;

// column1m_jvp_eval with the KP tangents of the constants.  The NaN rule is the primal's: a NaN in a state input → every tendency of the point, value and
// tangents, BEFORE the own flux is subtracted; a NaN in ρ or q_s → the flux of species s, value and tangents.
template <typename S, typename FT, int KP, typename CA>
__device__ __forceinline__ void column1m_param_eval(const CA &a0, const FT (&x)[S::NWRT + 1], FT inv_dz, ColumnPoint<FT, KP> &p) {
    using M = Math<FT>;
    const bool poison = S::poison(x);
    Dual<FT, KP> o[S::NOUT], F[4];
    S::template eval<FT, KP>(a0, x, o, F);
    p.g = S::g_of(x[0], inv_dz);
    for_each_slot<4>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        const bool fpoison = S::flux_poison(x, s);
        p.Fv[s] = S::out(F[s].v, fpoison);
        p.Av[s] = M::fma(-p.Fv[s], p.g, S::out(o[s].v, poison));      // minus the outflow through the lower face
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            p.Fd[k][s] = S::out(F[s].d[k], fpoison);
            p.Ad[k][s] = M::fma(-p.Fd[k][s], p.g, S::out(o[s].d[k], poison));
        }
    });
}

// ---- J_θ δθ -----------------------------------------------------------------------------------------------------------------------------------------
// `jvp[k][q]`: the column of direction slot k, output q; `jvp_precip[k][r]` (r = 0 rain, 1 snow): one value per column; `tend`, `precip`: the primal.
template <typename FT, int KP> struct Col1mParamJvpArgs {
    const FT *in[CMX_MP1M_JAC_NWRT + 1];      // rho, then the other inputs
    FT *tend[CMX_MP1M_JAC_NOUT];
    FT *precip[2];
    FT *jvp[KP][CMX_MP1M_JAC_NOUT];
    FT *jvp_precip[KP][2];
    const FT *inv_dz;
    int64_t n;                                 // n_col · n_lev
    int32_t n_lev;
};

// The arguments of the launch of the directions d0 … d0 + KP − 1; the primal outputs go with the first launch.  False if the launch has no output at all.
template <typename FT, int KP>
inline bool make_col1m_param_jvp_args(Col1mParamJvpArgs<FT, KP> &a, const FT *const (&in)[CMX_MP1M_JAC_NWRT + 1], const FT *inv_dz, int64_t n, int32_t n_lev, int d0,
                                      int ndir, FT *const *jvp, FT *const *jvp_precip_rai, FT *const *jvp_precip_sno, FT *const *tendencies, FT *precip_rai,
                                      FT *precip_sno) {
    a = Col1mParamJvpArgs<FT, KP>{};
    for (int j = 0; j < CMX_MP1M_JAC_NWRT + 1; ++j) a.in[j] = in[j];
    bool wanted = false;
    for (int q = 0; q < CMX_MP1M_JAC_NOUT; ++q) wanted |= (a.tend[q] = d0 == 0 && tendencies ? tendencies[q] : nullptr) != nullptr;
    wanted |= (a.precip[0] = d0 == 0 ? precip_rai : nullptr) != nullptr;
    wanted |= (a.precip[1] = d0 == 0 ? precip_sno : nullptr) != nullptr;
    for (int k = 0; k < KP && d0 + k < ndir; ++k) {
        for (int q = 0; q < CMX_MP1M_JAC_NOUT && jvp; ++q) wanted |= (a.jvp[k][q] = jvp[(d0 + k) * CMX_MP1M_JAC_NOUT + q]) != nullptr;
        if (jvp_precip_rai) wanted |= (a.jvp_precip[k][0] = jvp_precip_rai[d0 + k]) != nullptr;
        if (jvp_precip_sno) wanted |= (a.jvp_precip[k][1] = jvp_precip_sno[d0 + k]) != nullptr;
    }
    a.inv_dz = inv_dz;
    a.n = n;
    a.n_lev = n_lev;
    return wanted;
}

// The inflow through the upper face — the fluxes (upv, upd) the cell above sends down; nothing enters through the model top: a zero flux, multiplied out as in
// the primal — and the stores of point i of column `col` (column1m_jvp_store with KP tangents).
template <typename S, typename FT, int KP>
__device__ __forceinline__ void column1m_param_jvp_store(const Col1mParamJvpArgs<FT, KP> &a, const ColumnPoint<FT, KP> &p, const FT (&upv)[4], const FT (&upd)[KP][4],
                                                         bool top, bool surface, int64_t i, int64_t col) {
    using M = Math<FT>;
    for_each_slot<S::NOUT>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        const FT yv = M::fma(top ? FT(0) : upv[s], p.g, p.Av[s]);
        if (a.tend[s]) a.tend[s][i] = yv;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const FT yd = M::fma(top ? FT(0) : upd[k][s], p.g, p.Ad[k][s]);
            if (a.jvp[k][s]) a.jvp[k][s][i] = yd;
        }
    });
    if (surface) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (a.precip[r]) a.precip[r][col] = p.Fv[S::RAI + r];
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (a.jvp_precip[k][r]) a.jvp_precip[k][r][col] = p.Fd[k][S::RAI + r];
        }
    }
}

// ---- the gradient -----------------------------------------------------------------------------------------------------------------------------------
// `cot[q]`: the cotangent column of output q (NULL: absent), `cot_precip[r]`: one per column (NULL: absent); `lam[s]`: flux slot s has a multiplier at all;
// `nterm`: the terms of a point's sum.
template <typename FT> struct Col1mParamVjpArgs {
    const FT *in[CMX_MP1M_JAC_NWRT + 1];
    const FT *cot[CMX_MP1M_JAC_NOUT];
    const FT *cot_precip[2];
    FT *tend[CMX_MP1M_JAC_NOUT];
    FT *precip[2];
    const FT *inv_dz;
    int64_t n;
    int32_t n_lev;
    int32_t nterm;
    int32_t lam[4];
    int32_t primal;                   // tend or precip requested (the first launch only)
};

template <typename FT>
inline void make_col1m_param_vjp_args(Col1mParamVjpArgs<FT> &a, const FT *const (&in)[CMX_MP1M_JAC_NWRT + 1], const FT *inv_dz, int64_t n, int32_t n_lev,
                                      const FT *const *cotangents, const FT *cot_precip_rai, const FT *cot_precip_sno, bool first, FT *const *tendencies,
                                      FT *precip_rai, FT *precip_sno) {
    a = Col1mParamVjpArgs<FT>{};
    for (int j = 0; j < CMX_MP1M_JAC_NWRT + 1; ++j) a.in[j] = in[j];
    bool any = first && (precip_rai != nullptr || precip_sno != nullptr);
    for (int q = 0; q < CMX_MP1M_JAC_NOUT; ++q) {
        a.cot[q] = cotangents ? cotangents[q] : nullptr;
        a.tend[q] = first && tendencies ? tendencies[q] : nullptr;
        any |= a.tend[q] != nullptr;
        a.nterm += a.cot[q] != nullptr;
    }
    a.primal = any;
    a.cot_precip[0] = cot_precip_rai;
    a.cot_precip[1] = cot_precip_sno;
    a.precip[0] = first ? precip_rai : nullptr;
    a.precip[1] = first ? precip_sno : nullptr;
    a.inv_dz = inv_dz;
    a.n = n;
    a.n_lev = n_lev;
    for (int s = 0; s < 4; ++s) {
        a.lam[s] = a.cot[s] != nullptr || (s >= 2 && a.cot_precip[s - 2] != nullptr);
        a.nterm += a.lam[s];
    }
}

// One point of the gradient: pointwise plus ρ and ḡ of the level below, as column1m_vjp_point.  λ first, then ONE evaluation for the KP directions; per slot
// the sum is one chain of fma seeded with −0 (no term at all: +0) — the point sums with ḡ in output order, then the fluxes with λ in slot order — widened to
// double and added to the lane's accumulator.  A NaN in the state, in a cotangent of the point (p̄ counts for the level-0 point) or in what λ reads makes the
// sum NaN.
template <typename S, typename FT, int KP, typename CA>
__device__ __forceinline__ void column1m_param_vjp_point(const CA &a0, const Col1mParamVjpArgs<FT> &a, const FT (&x)[S::NWRT + 1], int64_t i, int64_t col, int32_t lev,
                                                         double (&acc)[KP]) {
    using M = Math<FT>;
    using products_detail::ld;
    const bool top = lev == a.n_lev - 1;
    const FT gk = S::g_of(x[0], a.inv_dz[lev]);
    FT lam[4] = {FT(0), FT(0), FT(0), FT(0)};
    int gnan = 0;
    column1m_lambda<S, FT>(a, x, gk, i, col, lev, lam, gnan);
    const bool poison = S::poison(x);
    Dual<FT, KP> o[S::NOUT], F[4];
    S::template eval<FT, KP>(a0, x, o, F);
    FT g[S::NOUT];
    int cnan = gnan;
    const int64_t ic = products_detail::after(i, F[3].v);
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) {
        g[q] = a.cot[q] ? ld(a.cot[q], ic) : FT(0);
        cnan |= (int)(g[q] != g[q]);      // bitwise on purpose: no branch
    }
    const bool bad = (bool)((int)poison | cnan);      // a NaN cotangent of the point poisons its tendencies and sums too
    if (a.primal) {
        // the primal entry's operations: t through the NaN rule, A = fma(−F, g, t), the inflow from the flux values of the raw point above, from the
        // constants that hold duals (its tangents are dead)
        FT up[4] = {FT(0), FT(0), FT(0), FT(0)};
        if (!top) {
            FT xu[S::NWRT + 1];
            xu[0] = ld(a.in[0], i + 1);
            xu[1] = xu[2] = FT(0);
#pragma unroll
            for (int s = 0; s < 4; ++s) xu[3 + s] = ld(a.in[3 + s], i + 1);
            Dual<FT, KP> Fu[4];
            S::template fluxes<FT, KP>(a0.vc, xu[0], xu[3], xu[4], xu[5], xu[6], Fu);
#pragma unroll
            for (int s = 0; s < 4; ++s) up[s] = S::out(Fu[s].v, S::flux_poison(xu, s));
        }
        for_each_slot<S::NOUT>([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            const FT Fv = S::out(F[s].v, S::flux_poison(x, s));
            const FT A = M::fma(-Fv, gk, S::out(o[s].v, bad));
            if (a.tend[s]) a.tend[s][i] = M::fma(top ? FT(0) : up[s], gk, A);
            if constexpr (s >= 2) {
                if (lev == 0 && a.precip[s - 2]) a.precip[s - 2][col] = Fv;
            }
        });
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        FT s = a.nterm ? -FT(0) : FT(0);
#pragma unroll
        for (int q = 0; q < S::NOUT; ++q)
            if (a.cot[q]) s = M::fma(g[q], o[q].d[k], s);
        for_each_slot<4>([&](auto fc) {
            constexpr int f = decltype(fc)::value;
            if (a.lam[f]) s = M::fma(lam[f], F[f].d[k], s);
        });
        acc[k] += (double)S::out(s, bad);
    }
}

}  // namespace cmx
