// cmx_mp1m_jacobian.hpp — what the device kernel (cmx_mp1m_jacobian.hip) and the host test build (tests/native/jacobian_1m_host.cpp, CMX_HOST_BUILD) share
// of the 1-moment tendency Jacobian: the tangents per pass, the table that maps tangent slots to inputs and columns, and ONE pass of the point function
// mp1m_point + mp1m_aggregate (cmx_mp1m.hpp) on the dual value type (cmx_dual.hpp).  No HIP in here.
#pragma once
#include <cstdint>

#include "../../include/cmx.h"
#include "cmx_dual.hpp"
#include "cmx_mp1m.hpp"

namespace cmx {

// Tangents carried per evaluation of the point function, per float type: tuning numbers (-DCMX_JAC1M_K_F32=…, -DCMX_JAC1M_K_F64=…).  A pass costs one primal
// plus K tangent evaluations, so fewer, wider passes issue fewer instructions in all, as long as the kernel keeps its waves and spills nothing.  3 / 2 from
// the register counts (Float32 K = 3: 142–162 VGPRs, three waves per SIMD; Float64 K = 2: 226–276, K = 3: 272–338, K = 6 spills): the table of DESIGN.md §9;
// tools/time_mp1m_jacobian.py times a build with another K (CMX_LIB).
#ifndef CMX_JAC1M_K_F32
#define CMX_JAC1M_K_F32 3
#endif
#ifndef CMX_JAC1M_K_F64
#define CMX_JAC1M_K_F64 2
#endif
template <typename FT> constexpr int kJac1mK = sizeof(FT) == 4 ? CMX_JAC1M_K_F32 : CMX_JAC1M_K_F64;
constexpr int kJac1mNOut = CMX_MP1M_JAC_NOUT, kJac1mNWrt = CMX_MP1M_JAC_NWRT;

// Tangent slot s = pass·K + k: `wrt[s]` = the differentiated input it is seeded on (cmx_mp1m_jac_wrt) or −1 for an idle slot of the last pass;
// `col[s][o]` = the column ∂out_o/∂in_wrt[s] (NULL: not wanted).  `tend`: the optional primal columns.
template <typename FT, int K> struct Mp1mJacArgs {
    static constexpr int SLOTS = (kJac1mNWrt + K - 1) / K * K;
    const FT *in[7];                  // rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno
    FT *tend[kJac1mNOut];
    FT *col[SLOTS][kJac1mNOut];
    int32_t wrt[SLOTS];
    int32_t npass;
};

// The slot table of a call: an input whose four columns are all NULL is not seeded, the others take the slots in the order of cmx_mp1m_jac_wrt.
// False if the call has no output column at all.
template <typename FT, int K> inline bool make_jac1m_args(Mp1mJacArgs<FT, K> &a, const FT *const (&in)[7], FT *const *jac, FT *const *tendencies) {
    a = Mp1mJacArgs<FT, K>{};
    for (int j = 0; j < 7; ++j) a.in[j] = in[j];
    bool any = false;
    for (int q = 0; q < kJac1mNOut; ++q) {
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        any |= a.tend[q] != nullptr;
    }
    int ns = 0;
    for (int s = 0; s < Mp1mJacArgs<FT, K>::SLOTS; ++s) a.wrt[s] = -1;
    for (int j = 0; j < kJac1mNWrt && jac; ++j) {
        bool wanted = false;
        for (int q = 0; q < kJac1mNOut; ++q) wanted |= jac[q * kJac1mNWrt + j] != nullptr;
        if (!wanted) continue;
        a.wrt[ns] = j;
        for (int q = 0; q < kJac1mNOut; ++q) a.col[ns][q] = jac[q * kJac1mNWrt + j];
        ++ns;
    }
    a.npass = ns > 0 ? (ns + K - 1) / K : 1;      // tendencies alone: one pass with every slot idle
    return any || ns > 0;
}

// ONE pass: the four tendencies of point x = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno) as duals whose tangent k is the derivative with respect to input
// a.wrt[pass·K + k] (cmx_mp1m_jac_wrt; −1: idle, the tangent is zero).  The clamps of the inputs (BMT:147-152; T is not clamped) are the point function's
// own and so part of the differentiated function; ρ enters as a constant: its tangents are structural zeros.  The value parts are
// mp1m_tendencies_point's results bit for bit (before its NaN rule, which the caller applies).
// keep(): the inputs are made opaque per pass, so that the compiler does not hoist the primal — which does not depend on the pass — out of the loop over
// the passes and keep every intermediate of the point function alive across it (cmx_sb2006_jacobian.hpp has the numbers).  Recomputing the primal is what
// forward mode costs per pass.
template <typename FT, int K, uint32_t FLAGS, typename C, typename A>
__device__ __forceinline__ void mp1m_jacobian_pass(const C &c, const A &a, int pass, const FT (&x)[7], Dual<FT, K> (&o)[kJac1mNOut]) {
    using D = Dual<FT, K>;
    // the six differentiated inputs, in the order of cmx_mp1m_jac_wrt: T, q_tot, q_lcl, q_icl, q_rai, q_sno = x[1 … 6]
    D in[kJac1mNWrt];
#pragma unroll
    for (int j = 0; j < kJac1mNWrt; ++j) {
        in[j].v = keep(x[j + 1]);
#pragma unroll
        for (int k = 0; k < K; ++k) in[j].d[k] = a.wrt[pass * K + k] == j ? FT(1) : FT(0);
    }
    // `c` is the kernel's constants argument: Float64 (and the run-time-flags Float32 instantiation) reads it through the kernel-argument segment, phase by
    // phase (cmx_math.hpp front_consts), from inside the pass, so that no constant is live across the loop over the passes
    const Mp1mSrc<D> p = mp1m_point<D, FLAGS>(front_consts<FT, FLAGS == kRuntimeFlags>(c), D(keep(x[0])), in[CMX_MP1M_JAC_WRT_T], in[CMX_MP1M_JAC_WRT_Q_TOT],
                                              in[CMX_MP1M_JAC_WRT_Q_LCL], in[CMX_MP1M_JAC_WRT_Q_ICL], in[CMX_MP1M_JAC_WRT_Q_RAI], in[CMX_MP1M_JAC_WRT_Q_SNO]);
    mp1m_aggregate<D>(p, o[CMX_MP1M_JAC_DQ_LCL_DT], o[CMX_MP1M_JAC_DQ_ICL_DT], o[CMX_MP1M_JAC_DQ_RAI_DT], o[CMX_MP1M_JAC_DQ_SNO_DT]);
}

// every pass of one point, and its stores: the body of the kernel's lane and of the host loop
template <typename FT, int K, uint32_t FLAGS, typename C, typename A>
__device__ __forceinline__ void mp1m_jacobian_point(const C &c, const A &a, const FT (&x)[7], int64_t i) {
    // the poison rule of the 1-moment entries (mp1m_tendencies_point): a NaN in any input column — in Float64 also ρ ≤ 0 (cmx_math.hpp bad_density) — gives NaN
    // in every output of the point
    const bool bad = (bool)((int)any_nan(x[0], x[2], x[3], x[4], x[5], x[6], x[1]) | (int)bad_density(x[0]));
    for (int pass = 0; pass < a.npass; ++pass) {
        Dual<FT, K> o[kJac1mNOut];
        mp1m_jacobian_pass<FT, K, FLAGS>(c, a, pass, x, o);
        if (pass == 0) {
#pragma unroll
            for (int q = 0; q < kJac1mNOut; ++q)
                if (a.tend[q]) a.tend[q][i] = bad ? Math<FT>::nan() : o[q].v;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int q = 0; q < kJac1mNOut; ++q) {
                FT *const col = a.col[pass * K + k][q];
                if (col) col[i] = bad ? Math<FT>::nan() : o[q].d[k];
            }
        }
    }
}

}  // namespace cmx
