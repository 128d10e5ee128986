// cmx_mp2m_p3_column.hpp — what the two 2M + P3 column translation units share (cmx_mp2m_p3_column.hip: include/cmx.h (9b), the explicit flux divergence;
// cmx_mp2m_p3_column_implicit.hip: §(24), backward-Euler sedimentation): the species and input enums, the ONE flux function of a raw point — the fluxes and the
// fall speeds it multiplies into them — and the entry layer: the checks of (9b) in their order, steps (1) and (2) as the library's own launches, and the last
// launch passed as a callable, as cmx_column_implicit.hpp does for §(20)/(21).  The kernels, their IO structs and launches and the extern "C" functions stay in
// the two files.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cmx_launch.hpp"
#include "cmx_sb2006.hpp"

namespace cmx {

// species in the order of the tendency columns
enum : int { SP_QLCL = 0, SP_NLCL, SP_QRAI, SP_NRAI, SP_QICE, SP_NICE, SP_QRIM, SP_BRIM, SP_N };
// the host array `in` of the entries
enum : int { IN_RHO = 0, IN_T, IN_QTOT, IN_QLCL, IN_NLCL, IN_QRAI, IN_NRAI, IN_QICE, IN_NICE, IN_QRIM, IN_BRIM, IN_GUESS, IN_SHIFT };

// The downward fluxes ρ χ w of ONE raw point (clamp_to_nonneg as in the tendencies, BMT:912-921) and the fall speeds w multiplied into them — the only place
// they are formed: a lane's own points and the point after a launch's last tile of (9b), and every point of §(24), go through it.  Rain: the PSD and fall
// speeds of sed_fluxes_of_point (cmx_sb2006_column.hip), the same inline functions on the same operands.  Ice: the fall speeds of step (1).
// w: vt_m, vt_n (rain), v_m, v_n, v_m, v_m (q_ice, n_ice, q_rim, b_rim), with CLOUD vc_m, vc_n, else 0 — the values themselves, not F/(ρχ).
// NaN rule: a NaN in ρ or in a column a species' flux depends on gives a NaN flux — rain (q_rai, n_rai: both speeds come from both moments),
// ice (q_ice, n_ice, q_rim, b_rim, v_n, v_m: the four ice species share the two fall speeds), cloud (q_lcl, n_lcl).
template <typename FT, bool LIMITED, int VEL, bool CLOUD, typename C>
__device__ __forceinline__ void p3col_fluxes_of_point(const C &c, const CloudVelConsts<FT> &cv, FT rho, FT q_lcl, FT n_lcl, FT q_rai, FT n_rai, FT q_ice,
                                                      FT n_ice, FT q_rim, FT b_rim, FT v_n, FT v_m, FT (&f)[SP_N], FT (&w)[SP_N]) {
    using M = Math<FT>;
    const FT eps = M::eps();
    const FT r_ = max0(rho);
    {
        const FT qr = max0(q_rai), nr = max0(n_rai);
        const FT rs_rho = M::rsqrt(r_);
        const FT N_rai = r_ * nr;
        const FT L_rai = r_ * M::max(qr, eps);
        const SbRainPsd<FT> psd = sb2006_rain_psd<FT, LIMITED>(c, L_rai, M::max(N_rai, eps));
        FT vt_n, vt_m;
        sb2006_rain_velocity<FT, LIMITED, VEL>(c, r_, rs_rho, psd.l2_lam, N_rai < eps, qr < eps, vt_n, vt_m);
        const bool bad = any_nan(rho, q_rai, n_rai);
        f[SP_QRAI] = bad ? M::nan() : (r_ * qr) * vt_m;
        f[SP_NRAI] = bad ? M::nan() : (r_ * nr) * vt_n;
        w[SP_QRAI] = vt_m;
        w[SP_NRAI] = vt_n;
    }
    {
        const bool bad = any_nan(rho, q_ice, n_ice, q_rim, b_rim, v_n, v_m);
        f[SP_QICE] = bad ? M::nan() : (r_ * max0(q_ice)) * v_m;
        f[SP_NICE] = bad ? M::nan() : (r_ * max0(n_ice)) * v_n;
        f[SP_QRIM] = bad ? M::nan() : (r_ * max0(q_rim)) * v_m;
        f[SP_BRIM] = bad ? M::nan() : (r_ * max0(b_rim)) * v_m;
        w[SP_QICE] = v_m;
        w[SP_NICE] = v_n;
        w[SP_QRIM] = v_m;
        w[SP_BRIM] = v_m;
    }
    f[SP_QLCL] = FT(0);
    f[SP_NLCL] = FT(0);
    w[SP_QLCL] = FT(0);
    w[SP_NLCL] = FT(0);
    if constexpr (CLOUD) {
        const FT ql = max0(q_lcl), nl = max0(n_lcl);
        FT vc_n, vc_m;
        sb2006_cloud_velocity(cv, ql, r_, r_ * nl, vc_n, vc_m);
        const bool bad = any_nan(rho, q_lcl, n_lcl);
        f[SP_QLCL] = bad ? M::nan() : (r_ * ql) * vc_m;
        f[SP_NLCL] = bad ? M::nan() : (r_ * nl) * vc_n;
        w[SP_QLCL] = vc_m;
        w[SP_NLCL] = vc_n;
    }
}

// ---- steps (1) and (2): the library's own entries of the float type -------------------------------------------------------------------------------------
// the four volumetric products ρ·(q_ice, n_ice, q_rim, b_rim) → tend[SP_QICE … SP_BRIM] (p3col_products_kernel, cmx_mp2m_p3_column.hip)
template <typename FT> int32_t p3col_launch_products(const FT *const *in, FT *const *tend, int64_t n, hipStream_t s);

inline int32_t p3col_shape_velocities(const cmx_p3_ice_params_f32 *ip, uint32_t flags, int32_t brent_iters, float p, int64_t n, const float *rq, const float *rn,
                                      const float *x3, const float *x4, const float *rho, const float *guess, float *loglam, float *v_n, float *v_m, void *st) {
    return cmx_p3_shape_terminal_velocities_f32(&ip->scheme, &ip->vel_ice, &ip->quad, flags, brent_iters, p, n, rq, rn, x3, x4, rho, guess, loglam, nullptr, v_n, v_m, st);
}
inline int32_t p3col_shape_velocities(const cmx_p3_ice_params_f64 *ip, uint32_t flags, int32_t brent_iters, double p, int64_t n, const double *rq, const double *rn,
                                      const double *x3, const double *x4, const double *rho, const double *guess, double *loglam, double *v_n, double *v_m, void *st) {
    return cmx_p3_shape_terminal_velocities_f64(&ip->scheme, &ip->vel_ice, &ip->quad, flags, brent_iters, p, n, rq, rn, x3, x4, rho, guess, loglam, nullptr, v_n, v_m, st);
}
inline int32_t p3col_tendencies(const cmx_warm_rain_2m_f32 *wr, const cmx_p3_ice_params_f32 *ip, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n,
                                const float *const *in, const float *loglam, float *const *out, void *st) {
    return cmx_microphysics_2m_p3_tendencies_f32(wr, ip, tps, flags, n, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10], loglam, in[12], out, st);
}
inline int32_t p3col_tendencies(const cmx_warm_rain_2m_f64 *wr, const cmx_p3_ice_params_f64 *ip, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n,
                                const double *const *in, const double *loglam, double *const *out, void *st) {
    return cmx_microphysics_2m_p3_tendencies_f64(wr, ip, tps, flags, n, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10], loglam, in[12], out, st);
}

// ---- the entry layer: the checks of (9b) in their order, then `extra_ok` (an argument of the calling entry alone — §(24): dt — already judged by the caller,
// CMX_ERR_BAD_ARG), all before any HIP call; steps (1) and (2); the constants of step (3).  `last(limited, velk, c, cv)` is the translation unit's: it builds
// the kernel's IO struct, launches the sedimentation kernel(s) and returns the status -----------------------------------------------------------------------
template <typename FT, typename WR, typename IP, typename TH, typename VL, typename ST, typename L>
inline int32_t p3_column_entry(const WR *wr, const IP *ip, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int32_t brent_iters, FT p,
                               int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, FT *const *tend, FT *loglam, FT *v_n, FT *v_m, bool extra_ok,
                               void *stream, L &&last) {
    constexpr uint32_t kP3 = CMX_P3_SLOPE_CONSTANT | CMX_P3_NO_ASPECT_RATIO | CMX_P3_RAIN_PDF_LIMITED;
    if (!wr || !ip || !tps || !vel || !in || !tend || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (flags & ~(uint32_t)(kP3 | CMX_P3COL_VEL_SB2006 | CMX_P3COL_VEL_CHEN2022)) return CMX_ERR_BAD_ARG;
    const bool sbv = flags & CMX_P3COL_VEL_SB2006, chv = flags & CMX_P3COL_VEL_CHEN2022;
    if (sbv == chv) return CMX_ERR_BAD_ARG;                      // exactly one rain fall-speed scheme
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    const int64_t n = n_col * (int64_t)n_lev;
    // the collision kernel of step (2) gives a workgroup as few as 4 states (collision_geometry, cmx_p3_collisions.hip): refused here, before any launch
    if (n > 4 * ((int64_t)0x7fffffff - 7)) return CMX_ERR_UNSUPPORTED;
    if (n == 0) return CMX_OK;
    if (!inv_dz || !loglam || !v_n || !v_m) return CMX_ERR_BAD_ARG;
    for (int k = 0; k <= IN_BRIM; ++k) if (!in[k]) return CMX_ERR_BAD_ARG;       // the warm start and the INPC shift are optional
    for (int q = 0; q < SP_N; ++q) if (!tend[q]) return CMX_ERR_BAD_ARG;
    const bool limited = (flags & CMX_P3_RAIN_PDF_LIMITED) != 0;
    if (limited && !sb_limiters_ok(*wr)) return CMX_ERR_BAD_ARG;                 // clamp_ordered needs ordered limiter pairs
    if (sbv && !sb_rain_vel_ok(*vel, limited)) return CMX_ERR_BAD_ARG;           // the not-limited SB2006 fall speed needs aR < bR
    // what steps (1) and (2) would refuse after the first launch was enqueued: the quadrature order and the quantile level
    if (ip->quad.n < 1 || ip->quad.n > CMX_QUAD_MAX || !(p > FT(0) && p < FT(0.5))) return CMX_ERR_BAD_ARG;
    if (!extra_ok) return CMX_ERR_BAD_ARG;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // (1) ρ·(q_ice, n_ice, q_rim, b_rim) → the last four tendency columns, then shape + fall speeds on them
    if (const int32_t e = p3col_launch_products<FT>(in, tend, n, s)) return e;
    if (const int32_t e = p3col_shape_velocities(ip, flags & (CMX_P3_SLOPE_CONSTANT | CMX_P3_NO_ASPECT_RATIO), brent_iters, p, n, tend[SP_QICE], tend[SP_NICE],
                                                 tend[SP_QRIM], tend[SP_BRIM], in[IN_RHO], in[IN_GUESS], loglam, v_n, v_m, stream))
        return e;
    // (2) the eight tendencies.  log λ is read only where ice is present (p3_collision_kernel: q_ice > ϵ, n_ice > ϵ and both products ≥ ϵ), which is
    // where step (1) solved for it: the −Inf of the other points goes in as it is and is never loaded
    if (const int32_t e = p3col_tendencies(wr, ip, tps, flags & kP3, n, in, loglam, tend, stream)) return e;
    // (3) fall speeds of rain (and cloud) + the sedimentation of the falling species
    const SbConsts<FT> c = make_sb_consts<FT>(*wr, *tps, vel, (double)Math<FT>::eps_1m());
    CloudVelConsts<FT> cv{};
    if (cloud_vel) cv = make_cloud_vel_consts<FT>(wr->seifert_beheng.pdf_c, *cloud_vel);
    const int velk = sbv ? VEL_SB : chen_vel_kind<FT>(vel->chen2022);   // fitted Γ(b(ρ)+1) or the general instantiation (cmx_math.hpp ChenGamma)
    return last(limited, velk, c, cv);
}

}  // namespace cmx
