// parcel_host.cpp — TEST INFRASTRUCTURE, like precip_susceptibility_host.cpp: the point functions of csrc/cmx_parcel.hpp (the parcel model's right-hand
// side and its forward-Euler step) with their host folding (make_parcel_consts) compiled by g++ for the HOST (CMX_HOST_BUILD: libm stand-ins for the
// hardware transcendental instructions), so that the algebra, the gates, the limiters and the NaN rule are checked in the CPU suite
// (tests/test_parcel_host.py).  Not part of libcmx.so; the -m gpu suite checks the device bits.
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../include/cmx.h"
#include "../../cloudmicrophysics.jl_amd/csrc/cmx_parcel.hpp"

namespace {
using namespace cmx;

template <typename FT> void load(const FT *const *state, const FT *w, const FT *const *coef, const ParcelConsts<FT> &c, int64_t i, FT (&Y)[9], FT &wi, FT (&k)[6]) {
    for (int j = 0; j < 9; ++j) Y[j] = state[j][i];
    wi = w[i];
    for (int j = 0; j < 6; ++j) k[j] = (coef && coef[j]) ? coef[j][i] : c.coef[j];
}

// the tendencies kernel's body per parcel: dY[9] and proc[6] columns, any NULL
template <typename FT, typename PP>
int32_t tendencies(const PP *pp, uint32_t flags, int64_t n, const FT *const *state, const FT *w, const FT *const *coef, FT *const *dY, FT *const *proc) {
    if (const int32_t st = parcel_flags_status(flags)) return st;
    const ParcelConsts<FT> c = make_parcel_consts<FT>(*pp, flags);
    for (int64_t i = 0; i < n; ++i) {
        FT Y[9], wi, k[6], d[9], r[6];
        load<FT>(state, w, coef, c, i, Y, wi, k);
        const bool bad = parcel_inputs_nan<FT>(Y, wi, k);
        parcel_rhs<FT>(c, flags, Y, wi, k, d, r);
        for (int j = 0; j < 9; ++j)
            if (dY && dY[j]) dY[j][i] = bad ? Math<FT>::nan() : d[j];
        for (int j = 0; j < 6; ++j)
            if (proc && proc[j]) proc[j][i] = bad ? Math<FT>::nan() : r[j];
    }
    return CMX_OK;
}

// the run kernel's body per parcel (no trajectory): n_steps Euler steps
template <typename FT, typename PP>
int32_t run(const PP *pp, uint32_t flags, int64_t n, int64_t n_steps, const FT *const *state, const FT *w, const FT *const *coef, FT *const *out) {
    if (const int32_t st = parcel_flags_status(flags)) return st;
    const ParcelConsts<FT> c = make_parcel_consts<FT>(*pp, flags);
    for (int64_t i = 0; i < n; ++i) {
        FT Y[9], wi, k[6];
        load<FT>(state, w, coef, c, i, Y, wi, k);
        if (parcel_inputs_nan<FT>(Y, wi, k))
            for (int j = 0; j < 9; ++j) Y[j] = Math<FT>::nan();
        for (int64_t s = 0; s < n_steps; ++s) parcel_step<FT>(c, flags, Y, wi, k);
        for (int j = 0; j < 9; ++j) out[j][i] = Y[j];
    }
    return CMX_OK;
}
}  // namespace

extern "C" {
int32_t parcel_tendencies_f32(const cmx_parcel_params_f32 *pp, uint32_t flags, int64_t n, const float *const *state, const float *w,
                              const float *const *coef, float *const *dY, float *const *proc) {
    return tendencies<float>(pp, flags, n, state, w, coef, dY, proc);
}
int32_t parcel_tendencies_f64(const cmx_parcel_params_f64 *pp, uint32_t flags, int64_t n, const double *const *state, const double *w,
                              const double *const *coef, double *const *dY, double *const *proc) {
    return tendencies<double>(pp, flags, n, state, w, coef, dY, proc);
}
int32_t parcel_run_f32(const cmx_parcel_params_f32 *pp, uint32_t flags, int64_t n, int64_t n_steps, const float *const *state, const float *w,
                       const float *const *coef, float *const *out) {
    return run<float>(pp, flags, n, n_steps, state, w, coef, out);
}
int32_t parcel_run_f64(const cmx_parcel_params_f64 *pp, uint32_t flags, int64_t n, int64_t n_steps, const double *const *state, const double *w,
                       const double *const *coef, double *const *out) {
    return run<double>(pp, flags, n, n_steps, state, w, coef, out);
}
}
