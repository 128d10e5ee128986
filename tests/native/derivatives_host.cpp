// derivatives_host.cpp — TEST INFRASTRUCTURE: the ONE host build of the derivative layer.  The driver of csrc/cmx_jacobian.hpp (slot tables, pass loop, the
// three point bodies jacobian_point / jvp_point / vjp_point) compiled by g++ for the HOST (CMX_HOST_BUILD: libm stand-ins for the hardware transcendental
// instructions, no kernel-argument tricks) on three schemes — SbJac (csrc/cmx_sb2006_jacobian.hpp), Mp1mJac (csrc/cmx_mp1m_jacobian.hpp), each set up by the
// function the device entries call (with_sb2006_jac / with_mp1m_jac), and a toy scheme that is NOT 4 × 6: 3 outputs, 5 differentiated inputs, sums and products
// only, so that on small-integer states every value and derivative is exact in both float types and can be asserted with ==.  The derivative rules are checked
// against finite differences of the oracle in the CPU suite without a GPU (tests/test_sb2006_jacobian_host.py, tests/test_mp1m_jacobian_host.py,
// tests/test_jacobian_driver_host.py), and unit-seed products against the Jacobian's columns and rows bit for bit (tests/test_jacobian_products_host.py).
// host_*_plain_* evaluates the PLAIN instantiation of the same point function with the tendencies kernel's sums: the dual's value parts must equal it bit for
// bit.  Like tests/native/point_host.cpp it is NOT part of libcmx.so and no CPU fallback.  The mirrors return the statuses of the device entries for what they
// check after the count rule: the flags and the limiter pairs, the tangent / cotangent table, "no output column at all".
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m_jacobian.hpp"
#include "../../cloudmicrophysics.jl_amd/csrc/cmx_sb2006_jacobian.hpp"

namespace {
using namespace cmx;

// The run-time tangent width k → the template argument K: the widths a scheme offers, as a selector of dispatch_or (an unlisted k misses).  k = 0: KDEF, the
// device kernel's own choice for the float type.  The columns do not depend on the width, bit for bit: each tangent is computed by the same operations whatever K is.
template <int... Ks> inline auto tangent_width(int k, int KDEF) { return one_of<Ks...>(k ? k : KDEF); }

// ---- the loops over the points: the body the device kernel's lane runs --------------------------------------------------------------------------
// x: the NWRT + 1 input columns; jac, tend: as the entry takes them.  False if the call has no output column at all.
template <typename S, typename FT, int K, typename C> bool host_jacobian_points(const C &c, int64_t n, const FT *const *x, FT *const *jac, FT *const *tend) {
    JacArgs<FT, K, S::NOUT, S::NWRT> a;
    const FT *in[S::NWRT + 1];
    for (int j = 0; j < S::NWRT + 1; ++j) in[j] = x[j];
    if (!make_jac_args(a, in, jac, tend)) return false;
    for (int64_t i = 0; i < n; ++i) {
        FT xi[S::NWRT + 1];
        for (int j = 0; j < S::NWRT + 1; ++j) xi[j] = a.in[j][i];
        jacobian_point<S, FT, K>(c, a, xi, i);
    }
    return true;
}

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
    return with_sb2006_jac<FT>(*wr, *tps, flags, [&](const SbConsts<FT> &c, auto S) {
        return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K) -> int32_t {
            return run<decltype(S), FT, decltype(K)::value>(what, c, n, x, p, q, tend) ? (int32_t)sb_integer_exponents(*wr) : (int32_t)CMX_ERR_BAD_ARG;
        }, tangent_width<1, 2, 3, 4, 6>(k, kJacK<FT>));
    });
}

// the plain instantiation: the sums of sb2006_tendencies_kernel (csrc/cmx_sb2006_kernels.hpp) around sb2006_point<FT, …, VEL_NONE, …>
template <typename FT, bool L, bool I> void sb2006_plain_points(SbJac<L, I>, const SbConsts<FT> &c, int64_t n, const FT *const *x, FT *const *y) {
    for (int64_t i = 0; i < n; ++i) {
        const FT rho = x[0][i], T = x[1][i], q_tot = x[2][i], q_lcl = x[3][i], n_lcl = x[4][i], q_rai = x[5][i], n_rai = x[6][i];
        const FT r_ = max0(rho), qt = max0(q_tot), ql = max0(q_lcl), qr = max0(q_rai), nl = max0(n_lcl), nr = max0(n_rai);
        const SbRates<FT> r = sb2006_point<FT, L, VEL_NONE, false, I>(c, r_, T, qt, ql, qr, r_ * nl, r_ * nr, nl, nr);
        const FT poison = any_nan(rho, q_tot, q_lcl, n_lcl, q_rai, n_rai, T) ? Math<FT>::nan() : FT(0);
        y[0][i] = ((r.cond + r.au_dq_lcl) + r.ac_dq_lcl) + poison;
        y[1][i] = Math<FT>::fma(r.lsc_plus_au + r.ac_dN_lcl, r.inv_rho, r.na_lcl) + poison;
        y[2][i] = ((r.evq + r.au_dq_rai) + r.ac_dq_rai) + poison;
        y[3][i] = Math<FT>::fma(((r.evN + r.au_dN_rai) + r.rsc) + r.rbr, r.inv_rho, r.na_rai) + poison;
    }
}
template <typename FT, typename WR, typename TH>
int32_t sb2006_plain(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const *x, FT *const *y) {
    return with_sb2006_jac<FT>(*wr, *tps, flags, [&](const SbConsts<FT> &c, auto S) {
        sb2006_plain_points(S, c, n, x, y);
        return (int32_t)sb_integer_exponents(*wr);
    });
}

// ---- 1-moment: returns 1 if the default-options / default-exponents instantiation ran, 0 for the run-time-flags one, or a status ------------------
template <uint32_t FLAGS> constexpr int32_t is_default(Mp1mJac<FLAGS>) { return FLAGS == kDefaultFlags; }

template <typename FT, typename MP, typename TH>
int32_t mp1m(int what, const MP *mp, const TH *tps, uint32_t flags, int k, int64_t n, const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {
    if (const int32_t st = check_flags_1m(flags)) return st;
    return with_mp1m_jac<FT>(*mp, *tps, flags, [&](const Mp1mConsts<FT> &c, auto S) {
        return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K) -> int32_t {
            return run<decltype(S), FT, decltype(K)::value>(what, c, n, x, p, q, tend) ? is_default(S) : (int32_t)CMX_ERR_BAD_ARG;
        }, tangent_width<1, 2, 3, 6>(k, kJac1mK<FT>));
    });
}

template <typename FT, uint32_t FLAGS> void mp1m_plain_points(Mp1mJac<FLAGS>, const Mp1mConsts<FT> &c, int64_t n, const FT *const *x, FT *const *y) {
    for (int64_t i = 0; i < n; ++i)
        mp1m_tendencies_point<FT, FLAGS>(c, x[0][i], x[1][i], x[2][i], x[3][i], x[4][i], x[5][i], x[6][i], y[0][i], y[1][i], y[2][i], y[3][i]);
}
template <typename FT, typename MP, typename TH>
int32_t mp1m_plain(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const *x, FT *const *y) {
    return with_mp1m_jac<FT>(*mp, *tps, flags, [&](const Mp1mConsts<FT> &c, auto S) {
        mp1m_plain_points(S, c, n, x, y);
        return is_default(S);
    });
}

// ---- the toy scheme: x = (rho, a, b, c, d, e):  o0 = ρ a b + c,  o1 = c d + w e + a,  o2 = a b c + d e ρ ------------------------------------------------
template <typename FT> struct ToyConsts { FT w; };
int64_t evals;      // evaluations of the scheme: passes × points
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
        ++evals;
    }
};
// k: 1 … 5 (0: 3).  The Jacobian returns the evaluations of the scheme per point = the passes that ran, the products CMX_OK
template <typename FT> int32_t toy(int what, FT w, int k, int64_t n, const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {
    const ToyConsts<FT> c{w};
    evals = 0;
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K) -> int32_t {
        if (!run<ToyJac, FT, decltype(K)::value>(what, c, n, x, p, q, tend)) return CMX_ERR_BAD_ARG;
        return what == 0 ? (int32_t)(evals / n) : (int32_t)CMX_OK;
    }, tangent_width<1, 2, 3, 4, 5>(k, 3));
}
}  // namespace

#define CMX_HOST_DERIVATIVES(SFX, FT)                                                                                                                \
    int32_t host_sb2006_derivative_##SFX(int what, const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, uint32_t flags, int k, int64_t n,  \
                                         const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {                                    \
        return sb2006<FT>(what, wr, tps, flags, k, n, x, p, q, tend);                                                                                \
    }                                                                                                                                                \
    int32_t host_sb2006_plain_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, uint32_t flags, int64_t n, const FT *const *x,    \
                                    FT *const *y) {                                                                                                  \
        return sb2006_plain<FT>(wr, tps, flags, n, x, y);                                                                                            \
    }                                                                                                                                                \
    int32_t host_mp1m_derivative_##SFX(int what, const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, uint32_t flags, int k, int64_t n, \
                                       const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {                                      \
        return mp1m<FT>(what, mp, tps, flags, k, n, x, p, q, tend);                                                                                  \
    }                                                                                                                                                \
    int32_t host_mp1m_plain_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, uint32_t flags, int64_t n, const FT *const *x,   \
                                  FT *const *y) {                                                                                                    \
        return mp1m_plain<FT>(mp, tps, flags, n, x, y);                                                                                              \
    }                                                                                                                                                \
    int32_t host_toy_derivative_##SFX(int what, FT w, int k, int64_t n, const FT *const *x, const FT *const *p, FT *const *q, FT *const *tend) {     \
        return toy<FT>(what, w, k, n, x, p, q, tend);                                                                                                \
    }

extern "C" {
int32_t host_jacobian_k_f32(void) { return kJacK<float>; }
int32_t host_jacobian_k_f64(void) { return kJacK<double>; }
int32_t host_jacobian_1m_k_f32(void) { return kJac1mK<float>; }
int32_t host_jacobian_1m_k_f64(void) { return kJac1mK<double>; }
CMX_HOST_DERIVATIVES(f32, float)
CMX_HOST_DERIVATIVES(f64, double)
}
