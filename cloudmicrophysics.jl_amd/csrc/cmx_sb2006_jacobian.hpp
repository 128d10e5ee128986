// cmx_sb2006_jacobian.hpp — what the device kernel (cmx_sb2006_jacobian.hip) and the host test build (tests/native/jacobian_host.cpp, CMX_HOST_BUILD) share
// of the SB2006 warm-rain Jacobian: the tangents per pass, the table that maps tangent slots to inputs and columns, and ONE pass of the point function on
// the dual value type (cmx_dual.hpp).  No HIP in here.
#pragma once
#include <cstdint>

#include "../../include/cmx.h"
#include "cmx_dual.hpp"
#include "cmx_sb2006.hpp"

namespace cmx {

// Tangents carried per evaluation of the point function, per float type: tuning numbers (-DCMX_JAC_K_F32=…, -DCMX_JAC_K_F64=…).  A pass costs one primal plus
// K tangent evaluations, so fewer, wider passes issue fewer instructions in all, as long as the kernel keeps its waves.  3 in both types: Float32 stays
// inside 128 VGPRs (four waves per SIMD), Float64 runs at one wave per SIMD from K = 2 on and K = 3 is two passes for all six inputs and one for up to three.
// The registers and measured times of K = 1, 2, 3, 6 are the table of DESIGN.md §9.
#ifndef CMX_JAC_K_F32
#define CMX_JAC_K_F32 3
#endif
#ifndef CMX_JAC_K_F64
#define CMX_JAC_K_F64 3
#endif
template <typename FT> constexpr int kJacK = sizeof(FT) == 4 ? CMX_JAC_K_F32 : CMX_JAC_K_F64;
constexpr int kJacNOut = CMX_SB2006_JAC_NOUT, kJacNWrt = CMX_SB2006_JAC_NWRT;

// Tangent slot s = pass·K + k: `wrt[s]` = the differentiated input it is seeded on (cmx_sb2006_jac_wrt) or −1 for an idle slot of the last pass;
// `col[s][o]` = the column ∂out_o/∂in_wrt[s] (NULL: not wanted).  `tend`: the optional primal columns.
template <typename FT, int K> struct SbJacArgs {
    static constexpr int SLOTS = (kJacNWrt + K - 1) / K * K;
    const FT *in[7];                  // rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai
    FT *tend[kJacNOut];
    FT *col[SLOTS][kJacNOut];
    int32_t wrt[SLOTS];
    int32_t npass;
};

// The slot table of a call: an input whose four columns are all NULL is not seeded, the others take the slots in the order of cmx_sb2006_jac_wrt.
// False if the call has no output column at all.
template <typename FT, int K> inline bool make_jac_args(SbJacArgs<FT, K> &a, const FT *const (&in)[7], FT *const *jac, FT *const *tendencies) {
    a = SbJacArgs<FT, K>{};
    for (int j = 0; j < 7; ++j) a.in[j] = in[j];
    bool any = false;
    for (int q = 0; q < kJacNOut; ++q) {
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        any |= a.tend[q] != nullptr;
    }
    int ns = 0;
    for (int s = 0; s < SbJacArgs<FT, K>::SLOTS; ++s) a.wrt[s] = -1;
    for (int j = 0; j < kJacNWrt && jac; ++j) {
        bool wanted = false;
        for (int q = 0; q < kJacNOut; ++q) wanted |= jac[q * kJacNWrt + j] != nullptr;
        if (!wanted) continue;
        a.wrt[ns] = j;
        for (int q = 0; q < kJacNOut; ++q) a.col[ns][q] = jac[q * kJacNWrt + j];
        ++ns;
    }
    a.npass = ns > 0 ? (ns + K - 1) / K : 1;      // tendencies alone: one pass with every slot idle
    return any || ns > 0;
}

// ONE pass: the four tendencies of point x = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai) as duals whose tangent k is the derivative with respect to input
// a.wrt[pass·K + k] (cmx_sb2006_jac_wrt; −1: idle, the tangent is zero).  The clamps, N = ρ n and the sums are sb2006_tendencies_kernel's (cmx_sb2006_kernels.hpp), so
// the value parts are that kernel's results bit for bit.
// keep(): the inputs are made opaque per pass.  Without it the compiler hoists the whole primal — which does not depend on the pass — out of the loop over
// the passes and keeps every intermediate of the point function alive across it: 192 instead of 128 VGPRs in Float32 at K = 3 with 31–53 spilled SGPRs,
// 338–360 instead of 272 in Float64 at K = 2 with 93–144 — and measured slower in Float32 (0.611 against 0.473 ms per 1e7 points; Float64 the same to
// 1 %).  Recomputing the primal is what forward mode costs per pass.
template <typename FT, int K, bool LIMITED, bool INTPOW, typename C, typename A>
__device__ __forceinline__ void sb2006_jacobian_pass(const C &c, const A &a, int pass, const FT (&x)[7], Dual<FT, K> (&o)[kJacNOut]) {
    using D = Dual<FT, K>;
    using MD = Math<D>;
    // the six differentiated inputs, in the order of cmx_sb2006_jac_wrt: T, q_tot, q_lcl, n_lcl, q_rai, n_rai = x[1 … 6]
    D in[kJacNWrt];
#pragma unroll
    for (int j = 0; j < kJacNWrt; ++j) {
        in[j].v = keep(x[j + 1]);
#pragma unroll
        for (int k = 0; k < K; ++k) in[j].d[k] = a.wrt[pass * K + k] == j ? FT(1) : FT(0);
    }
    // clamp_to_nonneg — BMT:828-837 (T is not clamped); the clamps are part of the differentiated function.  ρ is a constant: not differentiated
    const D r_ = D(max0(keep(x[0])));
    const D T = in[CMX_SB2006_JAC_WRT_T];
    const D qt = max0(in[CMX_SB2006_JAC_WRT_Q_TOT]), ql = max0(in[CMX_SB2006_JAC_WRT_Q_LCL]), nl = max0(in[CMX_SB2006_JAC_WRT_N_LCL]);
    const D qr = max0(in[CMX_SB2006_JAC_WRT_Q_RAI]), nr = max0(in[CMX_SB2006_JAC_WRT_N_RAI]);
    // N = ρ n — BMT:718-719.  `c` is the kernel's constants argument: Float64 reads it through the kernel-argument segment, phase by phase (cmx_math.hpp
    // front_consts), from inside the pass, so that no constant is live across the loop over the passes
    const SbRates<D> p = sb2006_point<D, LIMITED, VEL_NONE, false, INTPOW>(front_consts<FT>(c), r_, T, qt, ql, qr, r_ * nl, r_ * nr, nl, nr);
    o[CMX_SB2006_JAC_DQ_LCL_DT] = (p.cond + p.au_dq_lcl) + p.ac_dq_lcl;
    o[CMX_SB2006_JAC_DN_LCL_DT] = MD::fma(p.lsc_plus_au + p.ac_dN_lcl, p.inv_rho, p.na_lcl);
    o[CMX_SB2006_JAC_DQ_RAI_DT] = (p.evq + p.au_dq_rai) + p.ac_dq_rai;
    o[CMX_SB2006_JAC_DN_RAI_DT] = MD::fma(((p.evN + p.au_dN_rai) + p.rsc) + p.rbr, p.inv_rho, p.na_rai);
}

// every pass of one point, and its stores: the body of the kernel's lane and of the host loop
template <typename FT, int K, bool LIMITED, bool INTPOW, typename C, typename A>
__device__ __forceinline__ void sb2006_jacobian_point(const C &c, const A &a, const FT (&x)[7], int64_t i) {
    // a NaN in any input column poisons every output of the point (cmx_math.hpp any_nan): x + NaN = NaN, x + 0 = x
    const FT poison = any_nan(x[0], x[2], x[3], x[4], x[5], x[6], x[1]) ? Math<FT>::nan() : FT(0);
    for (int pass = 0; pass < a.npass; ++pass) {
        Dual<FT, K> o[kJacNOut];
        sb2006_jacobian_pass<FT, K, LIMITED, INTPOW>(c, a, pass, x, o);
        if (pass == 0) {
#pragma unroll
            for (int q = 0; q < kJacNOut; ++q)
                if (a.tend[q]) a.tend[q][i] = o[q].v + poison;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int q = 0; q < kJacNOut; ++q) {
                FT *const col = a.col[pass * K + k][q];
                if (col) col[i] = o[q].d[k] + poison;
            }
        }
    }
}

}  // namespace cmx
