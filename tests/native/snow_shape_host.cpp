// snow_shape_host.cpp — TEST INFRASTRUCTURE, like point_host.cpp: the shaped snow fall speed of csrc/cmx_mp1m_vel.hpp (vel_snow_shaped with the
// host-folded Vel1mShapeConsts of make_snow_shape_consts) compiled by g++ for the HOST (CMX_HOST_BUILD: libm stand-ins for the hardware
// transcendental instructions), so that the folding of CM1.aspect_ratio_coeffs into the log2-domain constants is checked in the CPU suite
// (tests/test_snow_shape_host.py).  Not part of libcmx.so; the -m gpu suite checks the device bits.
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m.hpp"
#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m_vel.hpp"

namespace {
using namespace cmx;
template <typename FT, typename CR, typename MP, typename CI>
int32_t snow_velocity(const MP *mp, const CI *chen_ice, uint32_t shape, int64_t n, const FT *rho, const FT *q, FT *w) {
    if (shape > CMX_SNOW_SHAPE_PROLATE) return CMX_ERR_BAD_ARG;
    const Vel1mShapeConsts<FT> c = make_snow_shape_consts<FT>(*mp, static_cast<const CR *>(nullptr), static_cast<const cmx_stokes_vel_f64 *>(nullptr),
                                                              *chen_ice, shape);
    for (int64_t i = 0; i < n; ++i) w[i] = vel_snow_shaped<FT>(c, rho[i], q[i]);
    return CMX_OK;
}
}  // namespace

extern "C" {
int32_t snow_velocity_f32(const cmx_microphysics_1m_f32 *mp, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t shape, int64_t n, const float *rho,
                          const float *q, float *w) {
    return snow_velocity<float, cmx_chen2022_rain_vel_f32>(mp, chen_ice, shape, n, rho, q, w);
}
int32_t snow_velocity_f64(const cmx_microphysics_1m_f64 *mp, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t shape, int64_t n, const double *rho,
                          const double *q, double *w) {
    return snow_velocity<double, cmx_chen2022_rain_vel_f64>(mp, chen_ice, shape, n, rho, q, w);
}
}
