// jacobian_products_host.cpp — TEST INFRASTRUCTURE: the products with the Jacobian of csrc/cmx_jacobian_products.hpp (jvp_point, vjp_point and their
// argument tables) compiled by g++ for the HOST (CMX_HOST_BUILD) on the three schemes the driver is tested with — SbJac (csrc/cmx_sb2006_jacobian.hpp),
// Mp1mJac (csrc/cmx_mp1m_jacobian.hpp) and the exact 3 × 5 toy scheme of jacobian_toy_host.cpp — next to the Jacobian itself and the plain instantiation
// in the SAME build, so that unit-seed products can be compared with the Jacobian's columns and rows bit for bit (tests/test_jacobian_products_host.py).
// Like the other host builds it is NOT part of libcmx.so and no CPU fallback.  The entry mirrors return the statuses of the device entries for what they
// check after the count rule: the tangent / cotangent table, "no output column at all", the flags and the limiter pairs.
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m_jacobian.hpp"
#include "../../cloudmicrophysics.jl_amd/csrc/cmx_sb2006_jacobian.hpp"
#include "jacobian_driver_host.hpp"

namespace {
using namespace cmx;

// ---- the loops over the points ------------------------------------------------------------------------------------------------------------------
template <typename S, typename FT, typename C>
bool host_jvp_points(const C &c, int64_t n, const FT *const *x, const FT *const *tan, FT *const *jvp, FT *const *tend) {
    JvpArgs<FT, S::NOUT, S::NWRT> a;
    const FT *in[S::NWRT + 1];
    for (int j = 0; j < S::NWRT + 1; ++j) in[j] = x[j];
    if (!tan || !make_jvp_args(a, in, tan, jvp, tend)) return false;
    for (int64_t i = 0; i < n; ++i) {
        FT xi[S::NWRT + 1], ti[S::NWRT];
        for (int j = 0; j < S::NWRT + 1; ++j) xi[j] = a.in[j][i];
        for (int j = 0; j < S::NWRT; ++j) ti[j] = a.tan[j] ? a.tan[j][i] : FT(0);
        jvp_point<S, FT>(c, a, xi, ti, i);
    }
    return true;
}

template <typename S, typename FT, int K, typename C>
bool host_vjp_points(const C &c, int64_t n, const FT *const *x, const FT *const *cot, FT *const *grad, FT *const *tend) {
    VjpArgs<FT, K, S::NOUT, S::NWRT> a;
    const FT *in[S::NWRT + 1];
    for (int j = 0; j < S::NWRT + 1; ++j) in[j] = x[j];
    if (!cot || !make_vjp_args(a, in, cot, grad, tend)) return false;
    for (int64_t i = 0; i < n; ++i) {
        FT xi[S::NWRT + 1];
        for (int j = 0; j < S::NWRT + 1; ++j) xi[j] = a.in[j][i];
        vjp_point<S, FT, K>(c, a, xi, i);
    }
    return true;
}

// what: 0 = the Jacobian (p = NULL, q = jac[24]), 1 = J v (p = tangents, q = jvp), 2 = Jᵀḡ (p = cotangents, q = grad)
template <typename S, typename FT, int K, typename C>
bool run(int what, const C &c, int64_t n, const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {
    if (what == 0) return host_jacobian_points<S, FT, K>(c, n, x, q, tend);
    if (what == 1) return host_jvp_points<S, FT>(c, n, x, p, q, tend);
    return host_vjp_points<S, FT, K>(c, n, x, p, q, tend);
}

// ---- SB2006: returns which instantiation ran (1 = the integer-exponent one) or a status ---------------------------------------------------------
template <typename FT, typename WR, typename TH>
int32_t sb2006(int what, const WR *wr, const TH *tps, uint32_t flags, int k, int64_t n, const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {
    if (flags & ~(uint32_t)CMX_SB2006_LIMITED) return CMX_ERR_BAD_ARG;
    const bool limited = flags & CMX_SB2006_LIMITED, intpow = sb_integer_exponents(*wr);
    if (limited && !sb_limiters_ok(*wr)) return CMX_ERR_BAD_ARG;
    const SbConsts<FT> c = make_sb_consts<FT>(*wr, *tps, (const std::conditional_t<std::is_same<FT, float>::value, cmx_rain_vel_f32, cmx_rain_vel_f64> *)nullptr,
                                              (double)Math<FT>::eps_1m());
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K, auto L, auto I) -> int32_t {
        using S = SbJac<decltype(L)::value, decltype(I)::value>;
        return run<S, FT, decltype(K)::value>(what, c, n, x, p, q, tend) ? (int32_t)intpow : (int32_t)CMX_ERR_BAD_ARG;
    }, tangent_width<1, 2, 3, 6>(k, kJacK<FT>), flag(limited), flag(intpow));
}

template <typename FT, typename WR, typename TH>
int32_t sb2006_plain(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const *x, FT *const *y) {
    const bool limited = flags & CMX_SB2006_LIMITED;
    if (limited && !sb_limiters_ok(*wr)) return CMX_ERR_BAD_ARG;
    const SbConsts<FT> c = make_sb_consts<FT>(*wr, *tps, (const std::conditional_t<std::is_same<FT, float>::value, cmx_rain_vel_f32, cmx_rain_vel_f64> *)nullptr,
                                              (double)Math<FT>::eps_1m());
    const bool intpow = sb_integer_exponents(*wr);
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto L, auto I) -> int32_t {
        for (int64_t i = 0; i < n; ++i) {
            const FT rho = x[0][i], T = x[1][i], q_tot = x[2][i], q_lcl = x[3][i], n_lcl = x[4][i], q_rai = x[5][i], n_rai = x[6][i];
            const FT r_ = max0(rho), qt = max0(q_tot), ql = max0(q_lcl), qr = max0(q_rai), nl = max0(n_lcl), nr = max0(n_rai);
            const SbRates<FT> r = sb2006_point<FT, decltype(L)::value, VEL_NONE, false, decltype(I)::value>(c, r_, T, qt, ql, qr, r_ * nl, r_ * nr, nl, nr);
            const FT poison = any_nan(rho, q_tot, q_lcl, n_lcl, q_rai, n_rai, T) ? Math<FT>::nan() : FT(0);
            y[0][i] = ((r.cond + r.au_dq_lcl) + r.ac_dq_lcl) + poison;
            y[1][i] = Math<FT>::fma(r.lsc_plus_au + r.ac_dN_lcl, r.inv_rho, r.na_lcl) + poison;
            y[2][i] = ((r.evq + r.au_dq_rai) + r.ac_dq_rai) + poison;
            y[3][i] = Math<FT>::fma(((r.evN + r.au_dN_rai) + r.rsc) + r.rbr, r.inv_rho, r.na_rai) + poison;
        }
        return intpow;
    }, flag(limited), flag(intpow));
}

// ---- 1-moment: returns 1 if the default-options / default-exponents instantiation ran, 0 for the run-time-flags one, or a status ------------------
template <typename FT, typename MP, typename TH>
int32_t mp1m(int what, const MP *mp, const TH *tps, uint32_t flags, int k, int64_t n, const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {
    if (const int32_t st = check_flags_1m(flags)) return st;
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(*mp, *tps, flags, (double)Math<FT>::eps_1m());
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K, auto FL) -> int32_t {
        constexpr uint32_t FLAGS = decltype(FL)::value;
        return run<Mp1mJac<FLAGS>, FT, decltype(K)::value>(what, c, n, x, p, q, tend) ? (int32_t)(FLAGS == kDefaultFlags) : (int32_t)CMX_ERR_BAD_ARG;
    }, tangent_width<1, 2, 3, 6>(k, kJac1mK<FT>), flags_1m(flags, c));
}

template <typename FT, typename MP, typename TH>
int32_t mp1m_plain(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const *x, FT *const *y) {
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(*mp, *tps, flags, (double)Math<FT>::eps_1m());
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto FL) -> int32_t {
        constexpr uint32_t FLAGS = decltype(FL)::value;
        for (int64_t i = 0; i < n; ++i)
            mp1m_tendencies_point<FT, FLAGS>(c, x[0][i], x[1][i], x[2][i], x[3][i], x[4][i], x[5][i], x[6][i], y[0][i], y[1][i], y[2][i], y[3][i]);
        return FLAGS == kDefaultFlags;
    }, flags_1m(flags, c));
}

// ---- the toy scheme of jacobian_toy_host.cpp: x = (rho, a, b, c, d, e):  o0 = ρ a b + c,  o1 = c d + w e + a,  o2 = a b c + d e ρ ----------------------
template <typename FT> struct ToyConsts { FT w; };
struct ToyJac {
    static constexpr int NOUT = 3, NWRT = 5;
    template <typename FT> static bool poison(const FT (&x)[NWRT + 1]) { return x[0] != x[0]; }
    template <typename FT> static FT out(FT v, bool bad) { return bad ? Math<FT>::nan() : v; }
    template <typename FT, int K, typename C> static void eval(const C &c, FT rho, const Dual<FT, K> (&in)[NWRT], Dual<FT, K> (&o)[NOUT]) {
        using D = Dual<FT, K>;
        const D r = D(rho), &a = in[0], &b = in[1], &cc = in[2], &d = in[3], &e = in[4];
        o[0] = r * a * b + cc;
        o[1] = cc * d + D(c.w) * e + a;
        o[2] = a * b * cc + d * e * r;
    }
};
template <typename FT> int32_t toy(int what, FT w, int k, int64_t n, const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {
    const ToyConsts<FT> c{w};
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K) -> int32_t {
        return run<ToyJac, FT, decltype(K)::value>(what, c, n, x, p, q, tend) ? (int32_t)CMX_OK : (int32_t)CMX_ERR_BAD_ARG;
    }, tangent_width<1, 2, 3, 4, 5>(k, 3));
}
}  // namespace

#define CMX_HOST_PRODUCTS(SFX, FT)                                                                                                                              \
    int32_t host_sb2006_product_##SFX(int what, const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, uint32_t flags, int k, int64_t n,               \
                                      const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {                                                \
        return sb2006<FT>(what, wr, tps, flags, k, n, x, p, q, tend);                                                                                           \
    }                                                                                                                                                           \
    int32_t host_sb2006_plain_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, uint32_t flags, int64_t n, const FT *const *x,             \
                                    FT *const *y) {                                                                                                           \
        return sb2006_plain<FT>(wr, tps, flags, n, x, y);                                                                                                       \
    }                                                                                                                                                           \
    int32_t host_mp1m_product_##SFX(int what, const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, uint32_t flags, int k, int64_t n,              \
                                    const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {                                                  \
        return mp1m<FT>(what, mp, tps, flags, k, n, x, p, q, tend);                                                                                             \
    }                                                                                                                                                           \
    int32_t host_mp1m_plain_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, uint32_t flags, int64_t n, const FT *const *x,            \
                                  FT *const *y) {                                                                                                             \
        return mp1m_plain<FT>(mp, tps, flags, n, x, y);                                                                                                         \
    }                                                                                                                                                           \
    int32_t host_toy_product_##SFX(int what, FT w, int k, int64_t n, const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {                 \
        return toy<FT>(what, w, k, n, x, p, q, tend);                                                                                                           \
    }

extern "C" {
CMX_HOST_PRODUCTS(f32, float)
CMX_HOST_PRODUCTS(f64, double)
}
