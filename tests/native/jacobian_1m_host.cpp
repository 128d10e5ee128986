// jacobian_1m_host.cpp — TEST INFRASTRUCTURE: the 1-moment tendency Jacobian of csrc/cmx_mp1m_jacobian.hpp — mp1m_point + mp1m_aggregate instantiated on the
// dual value type of csrc/cmx_dual.hpp, with the slot table and the per-point body the device kernel runs — compiled by g++ for the HOST (CMX_HOST_BUILD:
// libm stand-ins for the hardware transcendental instructions, no kernel-argument tricks), so that the derivative rules can be checked against finite
// differences of the oracle in the CPU suite (tests/test_mp1m_jacobian_host.py) without a GPU.  Like tests/native/point_host.cpp it is NOT part of
// libcmx.so and no CPU fallback.  host_mp1m_plain_* evaluates the PLAIN instantiation (mp1m_tendencies_point): the dual's value parts must equal it bit
// for bit.
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m_jacobian.hpp"
#include "jacobian_driver_host.hpp"

namespace {
using namespace cmx;

// k: the tangents per pass (jacobian_driver_host.hpp).
// Returns 1 if the default-options / default-exponents instantiation ran, 0 for the run-time-flags one (the choice of flags_1m)
template <typename FT, typename MP, typename TH>
int32_t jacobian(const MP *mp, const TH *tps, uint32_t flags, int k, int64_t n, const FT *const *x, FT *const *jac, FT *const *tend) {
    if (const int32_t st = check_flags_1m(flags)) return st;
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(*mp, *tps, flags, (double)Math<FT>::eps_1m());
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K, auto FL) -> int32_t {
        constexpr uint32_t FLAGS = decltype(FL)::value;
        return host_jacobian_points<Mp1mJac<FLAGS>, FT, decltype(K)::value>(c, n, x, jac, tend) ? (int32_t)(FLAGS == kDefaultFlags) : (int32_t)CMX_ERR_BAD_ARG;
    }, tangent_width<1, 2, 3, 6>(k, kJac1mK<FT>), flags_1m(flags, c));
}

template <typename FT, typename MP, typename TH>
int32_t plain(const MP *mp, const TH *tps, uint32_t flags, int64_t n, const FT *const *x, FT *const *y) {
    const Mp1mConsts<FT> c = make_mp1m_consts<FT>(*mp, *tps, flags, (double)Math<FT>::eps_1m());
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto FL) -> int32_t {
        constexpr uint32_t FLAGS = decltype(FL)::value;
        for (int64_t i = 0; i < n; ++i)
            mp1m_tendencies_point<FT, FLAGS>(c, x[0][i], x[1][i], x[2][i], x[3][i], x[4][i], x[5][i], x[6][i], y[0][i], y[1][i], y[2][i], y[3][i]);
        return FLAGS == kDefaultFlags;
    }, flags_1m(flags, c));
}
}  // namespace

extern "C" {
int32_t host_mp1m_jacobian_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int k, int64_t n, const float *const *x, float *const *jac, float *const *tend) { return jacobian<float>(mp, tps, flags, k, n, x, jac, tend); }
int32_t host_mp1m_jacobian_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int k, int64_t n, const double *const *x, double *const *jac, double *const *tend) { return jacobian<double>(mp, tps, flags, k, n, x, jac, tend); }
int32_t host_mp1m_plain_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n, const float *const *x, float *const *y) { return plain<float>(mp, tps, flags, n, x, y); }
int32_t host_mp1m_plain_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n, const double *const *x, double *const *y) { return plain<double>(mp, tps, flags, n, x, y); }
}
