// implicit_host.cpp — TEST INFRASTRUCTURE: the host build of the linearly implicit tendency r = (I − Δt J)⁻¹ f (csrc/cmx_jacobian.hpp: ImplicitArgs,
// make_implicit_args, implicit_point) compiled by g++ for the HOST (CMX_HOST_BUILD) on three schemes — SbJac and Mp1mJac, each set up by the function the
// device entries call (with_sb2006_jac / with_mp1m_jac), and a LINEAR toy scheme f = M s with the 4 × 4 matrix M handed in by the test, so that the solve
// alone — equilibration, pivoting, elimination — can be compared with a closed form (tests/test_implicit_host.py).  The Jacobian and the plain tendencies
// these are compared with come from tests/native/derivatives_host.cpp.  Like that file it is NOT part of libcmx.so and no CPU fallback.  The mirrors return
// the statuses of the device entries for what they check after the columns: the `implicit` table, Δt, "no output column at all", the flags and the limiters.
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m_jacobian.hpp"
#include "../../cloudmicrophysics.jl_amd/csrc/cmx_sb2006_jacobian.hpp"

namespace {
using namespace cmx;

// the loop over the points: the body the device kernel's lane runs.  False where the entry reports CMX_ERR_BAD_ARG after the columns
template <typename S, typename FT, int K, typename C> bool host_implicit_points(const C &c, double dt, int64_t n, const FT *const *x, FT *const *r, FT *const *tend) {
    ImplicitArgs<FT, K, S::NOUT, S::NWRT> a;
    const FT *in[S::NWRT + 1];
    for (int j = 0; j < S::NWRT + 1; ++j) in[j] = x[j];
    if (!r || !implicit_dt_ok(dt) || !make_implicit_args(a, in, S::SPECIES0, dt, r, tend)) return false;
    for (int64_t i = 0; i < n; ++i) {
        FT xi[S::NWRT + 1];
        for (int j = 0; j < S::NWRT + 1; ++j) xi[j] = a.in[j][i];
        implicit_point<S, FT, K>(c, a, xi, i);
    }
    return true;
}

// k = 0: the device kernel's own K for the float type
template <typename S, typename FT, typename C> int32_t run(const C &c, double dt, int k, int64_t n, const FT *const *x, FT *const *r, FT *const *tend) {
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K) -> int32_t {
        return host_implicit_points<S, FT, decltype(K)::value>(c, dt, n, x, r, tend) ? (int32_t)CMX_OK : (int32_t)CMX_ERR_BAD_ARG;
    }, one_of<1, 2, 4>(k ? k : kImplicitK<FT>));
}

template <typename FT, typename WR, typename TH>
int32_t sb2006(const WR *wr, const TH *tps, uint32_t flags, double dt, int k, int64_t n, const FT *const *x, FT *const *r, FT *const *tend) {
    // the order of the device entry: the table, Δt and "no output" come before the flags and the limiters
    if (!r || !implicit_dt_ok(dt)) return CMX_ERR_BAD_ARG;
    return with_sb2006_jac<FT>(*wr, *tps, flags, [&](const SbConsts<FT> &c, auto S) { return run<decltype(S), FT>(c, dt, k, n, x, r, tend); });
}

template <typename FT, typename MP, typename TH>
int32_t mp1m(const MP *mp, const TH *tps, uint32_t flags, double dt, int k, int64_t n, const FT *const *x, FT *const *r, FT *const *tend) {
    if (const int32_t st = check_flags_1m(flags)) return st;
    if (!r || !implicit_dt_ok(dt)) return CMX_ERR_BAD_ARG;
    return with_mp1m_jac<FT>(*mp, *tps, flags, [&](const Mp1mConsts<FT> &c, auto S) { return run<decltype(S), FT>(c, dt, k, n, x, r, tend); });
}

// ---- the toy scheme: x = (rho, s0 … s3), f = M s with M row-major in the constants; rho only carries the NaN rule ------------------------------------
template <typename FT> struct ToyConsts { FT M[16]; };
struct ToyLin {
    static constexpr int NOUT = 4, NWRT = 4, SPECIES0 = 0;
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
template <typename FT> int32_t toy(const FT *M, double dt, int k, int64_t n, const FT *const *x, FT *const *r, FT *const *tend) {
    ToyConsts<FT> c;
    for (int j = 0; j < 16; ++j) c.M[j] = M[j];
    return run<ToyLin, FT>(c, dt, k, n, x, r, tend);
}
}  // namespace

#define CMX_HOST_IMPLICIT(SFX, FT)                                                                                                                     \
    int32_t host_sb2006_implicit_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, uint32_t flags, double dt, int k, int64_t n,     \
                                       const FT *const *x, FT *const *r, FT *const *tend) {                                                            \
        return sb2006<FT>(wr, tps, flags, dt, k, n, x, r, tend);                                                                                       \
    }                                                                                                                                                  \
    int32_t host_mp1m_implicit_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, uint32_t flags, double dt, int k, int64_t n,    \
                                     const FT *const *x, FT *const *r, FT *const *tend) {                                                              \
        return mp1m<FT>(mp, tps, flags, dt, k, n, x, r, tend);                                                                                         \
    }                                                                                                                                                  \
    int32_t host_toy_implicit_##SFX(const FT *M, double dt, int k, int64_t n, const FT *const *x, FT *const *r, FT *const *tend) {                     \
        return toy<FT>(M, dt, k, n, x, r, tend);                                                                                                       \
    }

extern "C" {
int32_t host_implicit_k_f32(void) { return kImplicitK<float>; }
int32_t host_implicit_k_f64(void) { return kImplicitK<double>; }
CMX_HOST_IMPLICIT(f32, float)
CMX_HOST_IMPLICIT(f64, double)
}
