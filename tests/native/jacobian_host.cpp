// jacobian_host.cpp — TEST INFRASTRUCTURE: the SB2006 warm-rain Jacobian of csrc/cmx_sb2006_jacobian.hpp — sb2006_point instantiated on the dual value type
// of csrc/cmx_dual.hpp, with the slot table and the per-point body the device kernel runs — compiled by g++ for the HOST (CMX_HOST_BUILD: libm stand-ins for
// the hardware transcendental instructions, no kernel-argument tricks), so that the derivative rules can be checked against finite differences of the oracle
// in the CPU suite (tests/test_sb2006_jacobian_host.py) without a GPU.  Like tests/native/point_host.cpp it is NOT part of libcmx.so and no CPU fallback.
// host_sb2006_plain_* evaluates the PLAIN instantiation of the same point function with the tendencies kernel's sums: the dual's value parts must equal it
// bit for bit.
#define CMX_HOST_BUILD 1
#include <cstdint>
#include <initializer_list>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_sb2006_jacobian.hpp"
#include "jacobian_driver_host.hpp"

namespace {
using namespace cmx;

// k: the tangents per pass (jacobian_driver_host.hpp).  Returns which instantiation ran: 1 = the integer-exponent one
template <typename FT, typename WR, typename TH>
int32_t jacobian(const WR *wr, const TH *tps, uint32_t flags, int k, int64_t n, const FT *const *x, FT *const *jac, FT *const *tend) {
    if (flags & ~(uint32_t)CMX_SB2006_LIMITED) return CMX_ERR_BAD_ARG;
    const bool limited = flags & CMX_SB2006_LIMITED, intpow = sb_integer_exponents(*wr);
    if (limited && !sb_limiters_ok(*wr)) return CMX_ERR_BAD_ARG;
    const SbConsts<FT> c = make_sb_consts<FT>(*wr, *tps, (const std::conditional_t<std::is_same<FT, float>::value, cmx_rain_vel_f32, cmx_rain_vel_f64> *)nullptr,
                                              (double)Math<FT>::eps_1m());
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K, auto L, auto I) -> int32_t {
        using S = SbJac<decltype(L)::value, decltype(I)::value>;
        return host_jacobian_points<S, FT, decltype(K)::value>(c, n, x, jac, tend) ? (int32_t)intpow : (int32_t)CMX_ERR_BAD_ARG;
    }, tangent_width<1, 2, 3, 4, 6>(k, kJacK<FT>), flag(limited), flag(intpow));
}

// the plain instantiation: the sums of sb2006_tendencies_kernel (csrc/cmx_sb2006_kernels.hpp) around sb2006_point<FT, …, VEL_NONE, …>
template <typename FT, typename WR, typename TH>
int32_t plain(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const *x, FT *const *y) {
    const bool limited = flags & CMX_SB2006_LIMITED;
    if (limited && !sb_limiters_ok(*wr)) return CMX_ERR_BAD_ARG;
    const SbConsts<FT> c = make_sb_consts<FT>(*wr, *tps, (const std::conditional_t<std::is_same<FT, float>::value, cmx_rain_vel_f32, cmx_rain_vel_f64> *)nullptr,
                                              (double)Math<FT>::eps_1m());
    const bool intpow = sb_integer_exponents(*wr);
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto L, auto I) -> int32_t {
        for (int64_t i = 0; i < n; ++i) {
            const FT rho = x[0][i], T = x[1][i], q_tot = x[2][i], q_lcl = x[3][i], n_lcl = x[4][i], q_rai = x[5][i], n_rai = x[6][i];
            const FT r_ = max0(rho), qt = max0(q_tot), ql = max0(q_lcl), qr = max0(q_rai), nl = max0(n_lcl), nr = max0(n_rai);
            const SbRates<FT> p = sb2006_point<FT, decltype(L)::value, VEL_NONE, false, decltype(I)::value>(c, r_, T, qt, ql, qr, r_ * nl, r_ * nr, nl, nr);
            const FT poison = any_nan(rho, q_tot, q_lcl, n_lcl, q_rai, n_rai, T) ? Math<FT>::nan() : FT(0);
            y[0][i] = ((p.cond + p.au_dq_lcl) + p.ac_dq_lcl) + poison;
            y[1][i] = Math<FT>::fma(p.lsc_plus_au + p.ac_dN_lcl, p.inv_rho, p.na_lcl) + poison;
            y[2][i] = ((p.evq + p.au_dq_rai) + p.ac_dq_rai) + poison;
            y[3][i] = Math<FT>::fma(((p.evN + p.au_dN_rai) + p.rsc) + p.rbr, p.inv_rho, p.na_rai) + poison;
        }
        return intpow;
    }, flag(limited), flag(intpow));
}
}  // namespace

extern "C" {
int32_t host_jacobian_k_f32(void) { return kJacK<float>; }
int32_t host_jacobian_k_f64(void) { return kJacK<double>; }
int32_t host_sb2006_jacobian_f32(const cmx_warm_rain_2m_f32 *wr, const cmx_thermo_f32 *tps, uint32_t flags, int k, int64_t n, const float *const *x, float *const *jac, float *const *tend) { return jacobian<float>(wr, tps, flags, k, n, x, jac, tend); }
int32_t host_sb2006_jacobian_f64(const cmx_warm_rain_2m_f64 *wr, const cmx_thermo_f64 *tps, uint32_t flags, int k, int64_t n, const double *const *x, double *const *jac, double *const *tend) { return jacobian<double>(wr, tps, flags, k, n, x, jac, tend); }
int32_t host_sb2006_plain_f32(const cmx_warm_rain_2m_f32 *wr, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n, const float *const *x, float *const *y) { return plain<float>(wr, tps, flags, n, x, y); }
int32_t host_sb2006_plain_f64(const cmx_warm_rain_2m_f64 *wr, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n, const double *const *x, double *const *y) { return plain<double>(wr, tps, flags, n, x, y); }
}
