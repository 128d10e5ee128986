// jacobian_toy_host.cpp — TEST INFRASTRUCTURE: the Jacobian driver of csrc/cmx_jacobian.hpp (slot table, pass loop, stores) on a toy scheme that is NOT
// 4 × 6 like the two real ones: 3 outputs, 5 differentiated inputs, sums and products only, so that on small-integer states every value and derivative is
// exact in Float32 and Float64 and the analytic Jacobian can be asserted with == (tests/test_jacobian_driver_host.py).  Compiled by g++ for the host.
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../include/cmx.h"
#include "jacobian_driver_host.hpp"

namespace {
using namespace cmx;

template <typename FT> struct ToyConsts { FT w; };
int64_t evals;      // evaluations of the scheme: passes × points

// x = (rho, a, b, c, d, e):  o0 = ρ a b + c,  o1 = c d + w e + a,  o2 = a b c + d e ρ
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

// k: the tangents per pass, 1 … 5 (0: 3).  Returns the evaluations of the scheme per point = the passes that ran
template <typename FT> int32_t jacobian(FT w, int k, int64_t n, const FT *const *x, FT *const *jac, FT *const *tend) {
    const ToyConsts<FT> c{w};
    evals = 0;
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K) -> int32_t {
        return host_jacobian_points<ToyJac, FT, decltype(K)::value>(c, n, x, jac, tend) ? (int32_t)(evals / n) : (int32_t)CMX_ERR_BAD_ARG;
    }, tangent_width<1, 2, 3, 4, 5>(k, 3));
}
}  // namespace

extern "C" {
int32_t host_toy_jacobian_f32(float w, int k, int64_t n, const float *const *x, float *const *jac, float *const *tend) { return jacobian<float>(w, k, n, x, jac, tend); }
int32_t host_toy_jacobian_f64(double w, int k, int64_t n, const double *const *x, double *const *jac, double *const *tend) { return jacobian<double>(w, k, n, x, jac, tend); }
}
