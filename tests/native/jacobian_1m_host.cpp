// jacobian_1m_host.cpp — TEST INFRASTRUCTURE: the 1-moment tendency Jacobian of csrc/cmx_mp1m_jacobian.hpp — mp1m_point + mp1m_aggregate instantiated on the
// dual value type of csrc/cmx_dual.hpp, with the slot table and the per-point body the device kernel runs — compiled by g++ for the HOST (CMX_HOST_BUILD:
// libm stand-ins for the hardware transcendental instructions, no kernel-argument tricks), so that the derivative rules can be checked against finite
// differences of the oracle in the CPU suite (tests/test_mp1m_jacobian_host.py) without a GPU.  Like tests/native/point_host.cpp it is NOT part of
// libcmx.so and no CPU fallback.  host_mp1m_plain_* evaluates the PLAIN instantiation (mp1m_tendencies_point): the dual's value parts must equal it bit
// for bit.
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m_jacobian.hpp"

namespace {
using namespace cmx;

// k: the tangents per pass (0: the kernel's own choice for the float type).  The columns do not depend on it, bit for bit.
// Returns 1 if the default-options / default-exponents instantiation ran, 0 for the run-time-flags one (the choice of flags_1m)
template <typename FT, int K, typename MP, typename TH>
int32_t jacobian_k(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const *x, FT *const *jac, FT *const *tend) {
    if (const int32_t st = check_flags_1m(flags)) return st;
    Mp1mJacArgs<FT, K> a;
    const FT *const in[7] = {x[0], x[1], x[2], x[3], x[4], x[5], x[6]};
    if (!make_jac1m_args<FT, K>(a, in, jac, tend)) return CMX_ERR_BAD_ARG;
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(*mp, *tps, flags, (double)Math<FT>::eps_1m());
    const bool def = flags == CMX_1M_DEFAULT_OPTIONS && mp1m_default_exponents(c);
    for (int64_t i = 0; i < n; ++i) {
        FT xi[7];
        for (int j = 0; j < 7; ++j) xi[j] = a.in[j][i];
        if (def) mp1m_jacobian_point<FT, K, kDefaultFlags>(c, a, xi, i);
        else mp1m_jacobian_point<FT, K, kRuntimeFlags>(c, a, xi, i);
    }
    return def ? 1 : 0;
}
template <typename FT, typename MP, typename TH>
int32_t jacobian(const MP *mp, const TH *tps, uint32_t flags, int k, int64_t n, const FT *const *x, FT *const *jac, FT *const *tend) {
    switch (k) {
        case 0: return jacobian_k<FT, kJac1mK<FT>>(mp, tps, flags, n, x, jac, tend);
        case 1: return jacobian_k<FT, 1>(mp, tps, flags, n, x, jac, tend);
        case 2: return jacobian_k<FT, 2>(mp, tps, flags, n, x, jac, tend);
        case 3: return jacobian_k<FT, 3>(mp, tps, flags, n, x, jac, tend);
        case 6: return jacobian_k<FT, 6>(mp, tps, flags, n, x, jac, tend);
        default: return CMX_ERR_BAD_ARG;
    }
}

template <typename FT, typename MP, typename TH>
int32_t plain(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const *x, FT *const *y) {
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(*mp, *tps, flags, (double)Math<FT>::eps_1m());
    const bool def = flags == CMX_1M_DEFAULT_OPTIONS && mp1m_default_exponents(c);
    for (int64_t i = 0; i < n; ++i) {
        if (def) mp1m_tendencies_point<FT, kDefaultFlags>(c, x[0][i], x[1][i], x[2][i], x[3][i], x[4][i], x[5][i], x[6][i], y[0][i], y[1][i], y[2][i], y[3][i]);
        else mp1m_tendencies_point<FT>(c, x[0][i], x[1][i], x[2][i], x[3][i], x[4][i], x[5][i], x[6][i], y[0][i], y[1][i], y[2][i], y[3][i]);
    }
    return def ? 1 : 0;
}
}  // namespace

extern "C" {
int32_t host_mp1m_jacobian_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int k, int64_t n, const float *const *x, float *const *jac, float *const *tend) { return jacobian<float>(mp, tps, flags, k, n, x, jac, tend); }
int32_t host_mp1m_jacobian_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int k, int64_t n, const double *const *x, double *const *jac, double *const *tend) { return jacobian<double>(mp, tps, flags, k, n, x, jac, tend); }
int32_t host_mp1m_plain_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n, const float *const *x, float *const *y) { return plain<float>(mp, tps, flags, n, x, y); }
int32_t host_mp1m_plain_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n, const double *const *x, double *const *y) { return plain<double>(mp, tps, flags, n, x, y); }
}
