// cmx_jacobian.hpp — the forward-mode Jacobian driver every Jacobian entry shares (cmx_sb2006_jacobian.hpp, cmx_mp1m_jacobian.hpp), on the device and in the
// host test builds (tests/native/jacobian_driver_host.hpp, CMX_HOST_BUILD): the table that maps tangent slots to inputs and columns, every pass of one point
// with its stores, and the kernel.  No HIP outside the guarded block at the end.
//
// A SCHEME is a struct of static members that supplies what differs between two entries:
//   NOUT, NWRT               outputs and differentiated inputs; a point is x[0] = ρ (held fixed) and x[1 … NWRT], the inputs in the order of the entry's wrt enum
//   eval<FT, K>(c, rho, in, o)   the clamps and the point function on Dual<FT, K> (cmx_dual.hpp): o[NOUT] from the seeded in[NWRT].  It reads the constants
//                            through front_consts (cmx_math.hpp) itself, from inside the pass, so that no constant is live across the loop over the passes
//   poison(x), out(v, p)     the entry's NaN rule: p = poison(x) once per point, every stored value and tangent goes through out(·, p)
// (tests/native/jacobian_toy_host.cpp is the smallest one.)
#pragma once
#include <cstdint>

#include "cmx_dual.hpp"

namespace cmx {

// Tangent slot s = pass·K + k: `wrt[s]` = the differentiated input it is seeded on (the entry's wrt enum) or −1 for an idle slot of the last pass;
// `col[s][o]` = the column ∂out_o/∂in_wrt[s] (NULL: not wanted).  `tend`: the optional primal columns.
template <typename FT, int K, int NOUT, int NWRT> struct JacArgs {
    static constexpr int SLOTS = (NWRT + K - 1) / K * K;
    const FT *in[NWRT + 1];           // rho, then the differentiated inputs
    FT *tend[NOUT];
    FT *col[SLOTS][NOUT];
    int32_t wrt[SLOTS];
    int32_t npass;
};

// The slot table of a call: an input whose NOUT columns are all NULL is not seeded, the others take the slots in the order of the wrt enum.
// False if the call has no output column at all.
template <typename FT, int K, int NOUT, int NWRT>
inline bool make_jac_args(JacArgs<FT, K, NOUT, NWRT> &a, const FT *const (&in)[NWRT + 1], FT *const *jac, FT *const *tendencies) {
    a = JacArgs<FT, K, NOUT, NWRT>{};
    for (int j = 0; j < NWRT + 1; ++j) a.in[j] = in[j];
    bool any = false;
    for (int q = 0; q < NOUT; ++q) {
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        any |= a.tend[q] != nullptr;
    }
    int ns = 0;
    for (int s = 0; s < JacArgs<FT, K, NOUT, NWRT>::SLOTS; ++s) a.wrt[s] = -1;
    for (int j = 0; j < NWRT && jac; ++j) {
        bool wanted = false;
        for (int q = 0; q < NOUT; ++q) wanted |= jac[q * NWRT + j] != nullptr;
        if (!wanted) continue;
        a.wrt[ns] = j;
        for (int q = 0; q < NOUT; ++q) a.col[ns][q] = jac[q * NWRT + j];
        ++ns;
    }
    a.npass = ns > 0 ? (ns + K - 1) / K : 1;      // tendencies alone: one pass with every slot idle
    return any || ns > 0;
}

// Every pass of one point, and its stores: the body of the kernel's lane and of the host loop.  A pass evaluates the scheme on duals whose tangent k is the
// derivative with respect to input a.wrt[pass·K + k] (−1: idle, the tangent is zero); ρ enters as a constant, its tangents are structural zeros.
// keep(): the inputs are made opaque per pass — x[1 … NWRT] first, then ρ.  Without it the compiler hoists the whole primal — which does not depend on the
// pass — out of the loop over the passes and keeps every intermediate of the point function alive across it: SB2006, 192 instead of 128 VGPRs in Float32 at
// K = 3 with 31–53 spilled SGPRs, 338–360 instead of 272 in Float64 at K = 2 with 93–144 — and measured slower in Float32 (0.611 against 0.473 ms per 1e7
// points; Float64 the same to 1 %).  Recomputing the primal is what forward mode costs per pass.
template <typename S, typename FT, int K, typename C>
__device__ __forceinline__ void jacobian_point(const C &c, const JacArgs<FT, K, S::NOUT, S::NWRT> &a, const FT (&x)[S::NWRT + 1], int64_t i) {
    const auto poison = S::poison(x);
    for (int pass = 0; pass < a.npass; ++pass) {
        Dual<FT, K> in[S::NWRT], o[S::NOUT];
#pragma unroll
        for (int j = 0; j < S::NWRT; ++j) {
            in[j].v = keep(x[j + 1]);
#pragma unroll
            for (int k = 0; k < K; ++k) in[j].d[k] = a.wrt[pass * K + k] == j ? FT(1) : FT(0);
        }
        S::template eval<FT, K>(c, keep(x[0]), in, o);
        if (pass == 0) {
#pragma unroll
            for (int q = 0; q < S::NOUT; ++q)
                if (a.tend[q]) a.tend[q][i] = S::out(o[q].v, poison);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int q = 0; q < S::NOUT; ++q) {
                FT *const col = a.col[pass * K + k][q];
                if (col) col[i] = S::out(o[q].d[k], poison);
            }
        }
    }
}

#if !defined(CMX_HOST_BUILD)
// One point per lane.  `c`, the scheme's constants struct, stays the FIRST kernel argument: front_consts reads it at offset 0 of the kernel-argument segment.
template <typename S, typename FT, int K, int BS, typename C>
__global__ __launch_bounds__(BS) void jacobian_kernel(const C c, const JacArgs<FT, K, S::NOUT, S::NWRT> a, const int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    FT x[S::NWRT + 1];
    if (i < n) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS while the loads fly (every lane of the workgroup reaches the barrier inside); no-op for Float32
    if (i >= n) return;
    jacobian_point<S, FT, K>(c, a, x, i);
}
#endif

}  // namespace cmx

// J v and Jᵀḡ fused into the same pass: jvp_point / jvp_kernel, vjp_point / vjp_kernel
#include "cmx_jacobian_products.hpp"
