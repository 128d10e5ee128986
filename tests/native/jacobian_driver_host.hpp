// jacobian_driver_host.hpp — TEST INFRASTRUCTURE shared by the host builds of the Jacobian entries (jacobian_host.cpp, jacobian_1m_host.cpp,
// jacobian_toy_host.cpp): the run-time tangent width k → the template argument K, and the loop over the points through jacobian_point<Scheme, FT, K>
// (csrc/cmx_jacobian.hpp), the body the device kernel's lane runs.  Include it after #define CMX_HOST_BUILD 1 and the scheme's header.
#pragma once
#include <cstdint>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_dispatch.hpp"
#include "../../cloudmicrophysics.jl_amd/csrc/cmx_jacobian.hpp"

namespace cmx {

// The widths a build offers, as a selector of dispatch_or (an unlisted k misses).  k = 0: KDEF, the device kernel's own choice for the float type.
// The columns do not depend on the width, bit for bit: each tangent is computed by the same operations whatever K is.
template <int... Ks> inline auto tangent_width(int k, int KDEF) { return one_of<Ks...>(k ? k : KDEF); }

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

}  // namespace cmx
