// implicit_average_host.cpp — TEST INFRASTRUCTURE: the host build of the sub-stepped implicit average (csrc/cmx_jacobian.hpp: ImplicitAverageArgs,
// implicit_average_step_ok, make_implicit_average_args, implicit_average_point and through it implicit_average_substeps: the substep loop that the average
// kernel and the column kernel of cmx_column_implicit_step.hip both call, so this build covers the loop of both; the column kernel of
// cmx_column_implicit_average.hip keeps a measured copy, which only its device test holds to this one) compiled by g++ for the HOST (CMX_HOST_BUILD) on three schemes — SbJac and
// Mp1mJac, each set up by the function the device entries call (with_sb2006_jac / with_mp1m_jac), and a LINEAR toy scheme f = M s without a temperature, whose
// average has a closed form (tests/test_implicit_average_host.py).  What it is compared with, the recipe over the implicit entry, comes from
// tests/native/implicit_host.cpp.  Like that file it is NOT part of libcmx.so and no CPU fallback.  The mirrors return the statuses of the device entries for
// what they check after the columns: the `average` table, Δt, nsub, the step flags, "no output column at all", the flags and the limiters.
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m_jacobian.hpp"
#include "../../cloudmicrophysics.jl_amd/csrc/cmx_sb2006_jacobian.hpp"

namespace {
using namespace cmx;

template <typename FT> struct Step { double dt; int32_t nsub; uint32_t flags; FT LH_v0, LH_s0, cp_d; };

// the loop over the points: the body the device kernel's lane runs.  False where the entry reports CMX_ERR_BAD_ARG after the columns
template <typename S, typename FT, int K, typename C> bool host_average_points(const C &c, const Step<FT> &st, int64_t n, const FT *const *x, FT *const *avg) {
    ImplicitAverageArgs<FT, K, S::NOUT, S::NWRT> a;
    const FT *in[S::NWRT + 1];
    for (int j = 0; j < S::NWRT + 1; ++j) in[j] = x[j];
    if (!avg || !implicit_average_step_ok<FT>(st.dt, st.nsub, st.flags) ||
        !make_implicit_average_args(a, in, S::SPECIES0, st.dt, st.nsub, st.flags, st.LH_v0, st.LH_s0, st.cp_d, avg))
        return false;
    for (int64_t i = 0; i < n; ++i) {
        FT xi[S::NWRT + 1];
        for (int j = 0; j < S::NWRT + 1; ++j) xi[j] = a.in[j][i];
        implicit_average_point<S, FT, K>(c, a, xi, i);
    }
    return true;
}

// k = 0: the device kernel's own K for the float type
template <typename S, typename FT, typename C> int32_t run(const C &c, const Step<FT> &st, int k, int64_t n, const FT *const *x, FT *const *avg) {
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K) -> int32_t {
        return host_average_points<S, FT, decltype(K)::value>(c, st, n, x, avg) ? (int32_t)CMX_OK : (int32_t)CMX_ERR_BAD_ARG;
    }, one_of<1, 2, 4>(k ? k : kImplicitAvgK<FT>));
}

template <typename FT, typename WR, typename TH>
int32_t sb2006(const WR *wr, const TH *tps, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags, int k, int64_t n, const FT *const *x, FT *const *avg) {
    // the order of the device entry: the table, the step and "no output" come before the flags and the limiters
    const Step<FT> st{dt, nsub, step_flags, (FT)tps->LH_v0, (FT)tps->LH_s0, (FT)tps->cp_d};
    if (!avg || !implicit_average_step_ok<FT>(dt, nsub, step_flags)) return CMX_ERR_BAD_ARG;
    return with_sb2006_jac<FT>(*wr, *tps, flags, [&](const SbConsts<FT> &c, auto S) { return run<decltype(S), FT>(c, st, k, n, x, avg); });
}

template <typename FT, typename MP, typename TH>
int32_t mp1m(const MP *mp, const TH *tps, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags, int k, int64_t n, const FT *const *x, FT *const *avg) {
    const Step<FT> st{dt, nsub, step_flags, (FT)tps->LH_v0, (FT)tps->LH_s0, (FT)tps->cp_d};
    if (const int32_t rc = check_flags_1m(flags)) return rc;
    if (!avg || !implicit_average_step_ok<FT>(dt, nsub, step_flags)) return CMX_ERR_BAD_ARG;
    return with_mp1m_jac<FT>(*mp, *tps, flags, [&](const Mp1mConsts<FT> &c, auto S) { return run<decltype(S), FT>(c, st, k, n, x, avg); });
}

// ---- the toy scheme: x = (rho, s0 … s3), f = M s with M row-major in the constants; no temperature (TEMP < 0: nothing is heated); rho only carries the NaN rule
template <typename FT> struct ToyConsts { FT M[16]; };
struct ToyLin {
    static constexpr int NOUT = 4, NWRT = 4, SPECIES0 = 0, TEMP = -1;
    template <typename FT> static bool poison(const FT (&x)[NWRT + 1]) {
        bool bad = false;
        for (int j = 0; j < NWRT + 1; ++j) bad |= x[j] != x[j];
        return bad;
    }
    template <typename FT> static FT out(FT v, bool bad) { return bad ? Math<FT>::nan() : v; }
    template <typename FT, int K, typename C> static void eval(const C &c, FT, const Dual<FT, K> (&in)[NWRT], Dual<FT, K> (&o)[NOUT]) {
        for (int q = 0; q < NOUT; ++q) {
            o[q] = c.M[4 * q] * in[0];
            for (int j = 1; j < NWRT; ++j) o[q] = o[q] + c.M[4 * q + j] * in[j];
        }
    }
};
template <typename FT> int32_t toy(const FT *M, double dt, int32_t nsub, uint32_t step_flags, int k, int64_t n, const FT *const *x, FT *const *avg) {
    ToyConsts<FT> c;
    for (int j = 0; j < 16; ++j) c.M[j] = M[j];
    return run<ToyLin, FT>(c, Step<FT>{dt, nsub, step_flags, FT(0), FT(0), FT(1)}, k, n, x, avg);
}
}  // namespace

#define CMX_HOST_AVERAGE(SFX, FT)                                                                                                                              \
    int32_t host_sb2006_implicit_average_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, uint32_t flags, double dt, int32_t nsub,         \
                                               uint32_t step_flags, int k, int64_t n, const FT *const *x, FT *const *avg) {                                   \
        return sb2006<FT>(wr, tps, flags, dt, nsub, step_flags, k, n, x, avg);                                                                                 \
    }                                                                                                                                                          \
    int32_t host_mp1m_implicit_average_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, uint32_t flags, double dt, int32_t nsub,        \
                                             uint32_t step_flags, int k, int64_t n, const FT *const *x, FT *const *avg) {                                     \
        return mp1m<FT>(mp, tps, flags, dt, nsub, step_flags, k, n, x, avg);                                                                                   \
    }                                                                                                                                                          \
    int32_t host_toy_implicit_average_##SFX(const FT *M, double dt, int32_t nsub, uint32_t step_flags, int k, int64_t n, const FT *const *x, FT *const *avg) { \
        return toy<FT>(M, dt, nsub, step_flags, k, n, x, avg);                                                                                                 \
    }

extern "C" {
int32_t host_implicit_average_k_f32(void) { return kImplicitAvgK<float>; }
int32_t host_implicit_average_k_f64(void) { return kImplicitAvgK<double>; }
CMX_HOST_AVERAGE(f32, float)
CMX_HOST_AVERAGE(f64, double)
}
