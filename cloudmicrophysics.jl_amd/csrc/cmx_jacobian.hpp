// cmx_jacobian.hpp — the forward-mode derivative driver every scheme's entries share (cmx_sb2006_jacobian.hpp, cmx_mp1m_jacobian.hpp), on the device and in the
// host test build (tests/native/derivatives_host.cpp, CMX_HOST_BUILD): the table that maps tangent slots to inputs and, per operation — the Jacobian, J v,
// Jᵀḡ — the argument struct, every pass of one point with its stores, and the kernel.  No HIP outside the CMX_HOST_BUILD guards.
//
// A SCHEME is a struct of static members that supplies what differs between two entries:
//   NOUT, NWRT               outputs and differentiated inputs; a point is x[0] = ρ (held fixed) and x[1 … NWRT], the inputs in the order of the entry's wrt enum
//   eval<FT, K>(c, rho, in, o)   the clamps and the point function on Dual<FT, K> (cmx_dual.hpp): o[NOUT] from the seeded in[NWRT].  It reads the constants
//                            through front_consts (cmx_math.hpp) itself, from inside the pass, so that no constant is live across the loop over the passes
//   poison(x), out(v, p)     the entry's NaN rule: p = poison(x) once per point, every stored value and tangent goes through out(·, p)
// (ToyJac of tests/native/derivatives_host.cpp is the smallest one.)
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

// The slot table of a call: fills `wrt` and `npass` and returns the seeded slots.  An input that is not wanted(j) is not seeded, the others take the slots
// in the order of the wrt enum.
template <int K, int NWRT, int SLOTS, typename WANTED> inline int seed_slots(int32_t (&wrt)[SLOTS], int32_t &npass, WANTED &&wanted) {
    int ns = 0;
    for (int s = 0; s < SLOTS; ++s) wrt[s] = -1;
    for (int j = 0; j < NWRT; ++j)
        if (wanted(j)) wrt[ns++] = j;
    npass = ns > 0 ? (ns + K - 1) / K : 1;      // tendencies alone: one pass with every slot idle
    return ns;
}

// An input is wanted if one of its NOUT columns is not NULL.  False if the call has no output column at all.
template <typename FT, int K, int NOUT, int NWRT>
inline bool make_jac_args(JacArgs<FT, K, NOUT, NWRT> &a, const FT *const (&in)[NWRT + 1], FT *const *jac, FT *const *tendencies) {
    a = JacArgs<FT, K, NOUT, NWRT>{};
    for (int j = 0; j < NWRT + 1; ++j) a.in[j] = in[j];
    bool any = false;
    for (int q = 0; q < NOUT; ++q) {
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        any |= a.tend[q] != nullptr;
    }
    const int ns = seed_slots<K, NWRT>(a.wrt, a.npass, [&](int j) {
        bool wanted = false;
        for (int q = 0; q < NOUT && jac; ++q) wanted |= jac[q * NWRT + j] != nullptr;
        return wanted;
    });
    for (int s = 0; s < ns; ++s)
        for (int q = 0; q < NOUT; ++q) a.col[s][q] = jac[q * NWRT + a.wrt[s]];
    return any || ns > 0;
}

// Every pass of one point, and its stores: the body of the kernel's lane and of the host loop.  A pass evaluates the scheme on duals whose tangent k is the
// derivative with respect to input a.wrt[pass·K + k] (−1: idle, the tangent is zero); ρ enters as a constant, its tangents are structural zeros.
// keep(): the inputs are made opaque per pass — x[1 … NWRT] first, then ρ.  Without it the compiler hoists the whole primal — which does not depend on the
// pass — out of the loop over the passes and keeps every intermediate of the point function alive across it: SB2006, 192 instead of 128 VGPRs in Float32 at
// K = 3 with 31–53 spilled SGPRs, 338–360 instead of 272 in Float64 at K = 2 with 93–144 — and measured slower in Float32 (0.611 against 0.473 ms per 1e7
// points; Float64 the same to 1 %).  Recomputing the primal is what forward mode costs per pass.
// vjp_point below repeats the seeding and the call of eval on purpose.  Sharing them — as a for_each_pass(…, body) that takes the rest of the pass as a lambda, or
// as a plain __forceinline__ function for the seeding alone — compiled to other Float32 code at K = 3: +13 / +14 instructions in the SB2006 and 1-moment Jacobian
// kernels, up to +10 and 31 → 33 spilled SGPRs in the SB2006 Jᵀḡ kernel (Float64 was unchanged).
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

// ---- The two products with the Jacobian, fused into the pass that holds the tangents in registers: J v (forward mode with the caller's tangent as the seed)
// and Jᵀḡ (the columns of the Jacobian contracted with the cotangent before anything is stored), on the SAME SCHEME structs.  Semantics:
//   * The products are plain IEEE arithmetic on the tangents the Jacobian entry would store: a zero cotangent times an infinite tangent is NaN, exactly
//     as contracting the Jacobian's columns gives.  A NULL cotangent column removes that output from the sum structurally; a NULL tangent column is a
//     zero tangent (a run-time zero: the dual rules compute with it like with any other value).
//   * Jᵀḡ accumulates over the non-NULL cotangents in output order: the first product, then Math<FT>::fma(ḡ_q, ∂out_q, g) (vjp_point has the form).  Each gradient is computed
//     from its own tangent slot only, so its value does not depend on which other gradients are requested, bit for bit — the property the Jacobian entry
//     has for its columns.  (Against a Jacobian column the sum of a single product is the column times ḡ; with ḡ = 1 the column itself.)
//   * The NaN rule of the library extends to the new inputs: a NaN in any state input, or in any GIVEN tangent or cotangent value of a point, gives NaN in
//     every output of that point — products and tendencies — and in that point only.  It goes through the scheme's own poison(): the point is judged as
//     if its ρ were NaN.
namespace products_detail {
// a column element: the state is touched once per sweep (non-temporal) on the device
template <typename FT> __device__ __forceinline__ FT ld(const FT *p, int64_t i) {
#if defined(CMX_HOST_BUILD)
    return p[i];
#else
    return __builtin_nontemporal_load(p + i);
#endif
}
// i, not before v is computed: an index the optimiser cannot hoist a load above the point function with (host build: the identity)
template <typename FT> __device__ __forceinline__ int64_t after(int64_t i, FT v) {
#if !defined(CMX_HOST_BUILD)
    asm volatile("" : "+v"(i) : "v"(v));
#endif
    return i;
}
// the scheme's poison of the point, with "one of the given tangent / cotangent values is a NaN" folded in as a NaN ρ
template <typename S, typename FT> __device__ __forceinline__ auto poison_with(const FT (&x)[S::NWRT + 1], bool extra_nan) {
    FT xp[S::NWRT + 1];
#pragma unroll
    for (int j = 0; j < S::NWRT + 1; ++j) xp[j] = x[j];
    xp[0] = extra_nan ? Math<FT>::nan() : x[0];
    return S::poison(xp);
}
}  // namespace products_detail

// ---- J v ------------------------------------------------------------------------------------------------------------------------------------------
// `tan[j]`: the tangent column of differentiated input j (NULL: zero).  `jvp[q]` = Σ_j ∂out_q/∂in_j · tan_j, `tend[q]` = the primal; both NULL-able.
template <typename FT, int NOUT, int NWRT> struct JvpArgs {
    const FT *in[NWRT + 1];           // rho, then the differentiated inputs
    const FT *tan[NWRT];
    FT *jvp[NOUT];
    FT *tend[NOUT];
};

// False if the call has no output column at all.  `tangents` is the caller's table of NWRT members (not NULL itself: the entry checks that).
template <typename FT, int NOUT, int NWRT>
inline bool make_jvp_args(JvpArgs<FT, NOUT, NWRT> &a, const FT *const (&in)[NWRT + 1], const FT *const *tangents, FT *const *jvp, FT *const *tendencies) {
    a = JvpArgs<FT, NOUT, NWRT>{};
    for (int j = 0; j < NWRT + 1; ++j) a.in[j] = in[j];
    for (int j = 0; j < NWRT; ++j) a.tan[j] = tangents ? tangents[j] : nullptr;
    bool any = false;
    for (int q = 0; q < NOUT; ++q) {
        a.jvp[q] = jvp ? jvp[q] : nullptr;
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        any |= a.jvp[q] != nullptr || a.tend[q] != nullptr;
    }
    return any;
}

// One evaluation of the scheme on Dual<FT, 1> whose tangent is the caller's: t[j] = the tangent value of input j at this point (0 where the column is
// NULL).  ρ enters as a constant.  keep(): as in jacobian_point, the inputs are opaque to the optimiser.
template <typename S, typename FT, typename C>
__device__ __forceinline__ void jvp_point(const C &c, const JvpArgs<FT, S::NOUT, S::NWRT> &a, const FT (&x)[S::NWRT + 1], const FT (&t)[S::NWRT], int64_t i) {
    int tnan = 0;
#pragma unroll
    for (int j = 0; j < S::NWRT; ++j) tnan |= (int)(t[j] != t[j]);      // bitwise on purpose: no branch
    const auto poison = products_detail::poison_with<S>(x, (bool)tnan);
    Dual<FT, 1> in[S::NWRT], o[S::NOUT];
#pragma unroll
    for (int j = 0; j < S::NWRT; ++j) {
        in[j].v = keep(x[j + 1]);
        in[j].d[0] = keep(t[j]);
    }
    S::template eval<FT, 1>(c, keep(x[0]), in, o);
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) {
        if (a.tend[q]) a.tend[q][i] = S::out(o[q].v, poison);
        if (a.jvp[q]) a.jvp[q][i] = S::out(o[q].d[0], poison);
    }
}

// ---- Jᵀ ḡ -----------------------------------------------------------------------------------------------------------------------------------------
// Tangent slot s = pass·K + k as in JacArgs: `wrt[s]` = the input it is seeded on or −1 (idle), `grad[s]` = the gradient column of that input.
// `cot[q]`: the cotangent column of output q (NULL: the output is not part of the sum).  `tend`: the optional primal columns.
template <typename FT, int K, int NOUT, int NWRT> struct VjpArgs {
    static constexpr int SLOTS = (NWRT + K - 1) / K * K;
    const FT *in[NWRT + 1];
    const FT *cot[NOUT];
    FT *tend[NOUT];
    FT *grad[SLOTS];
    int32_t wrt[SLOTS];
    int32_t npass;
    int32_t ncot;                     // the non-NULL members of cot
};

// An input is wanted if its gradient is not NULL.  False if the call has no output column at all.  `cotangents` is the caller's table of NOUT members (not NULL itself: the entry checks that).
template <typename FT, int K, int NOUT, int NWRT>
inline bool make_vjp_args(VjpArgs<FT, K, NOUT, NWRT> &a, const FT *const (&in)[NWRT + 1], const FT *const *cotangents, FT *const *grad, FT *const *tendencies) {
    a = VjpArgs<FT, K, NOUT, NWRT>{};
    for (int j = 0; j < NWRT + 1; ++j) a.in[j] = in[j];
    bool any = false;
    for (int q = 0; q < NOUT; ++q) {
        a.cot[q] = cotangents ? cotangents[q] : nullptr;
        a.ncot += a.cot[q] != nullptr;
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        any |= a.tend[q] != nullptr;
    }
    const int ns = seed_slots<K, NWRT>(a.wrt, a.npass, [&](int j) { return grad && grad[j]; });
    for (int s = 0; s < ns; ++s) a.grad[s] = grad[a.wrt[s]];
    return any || ns > 0;
}

// Every pass of one point: the pass of jacobian_point, then — instead of NOUT stores per slot — the contraction with the cotangents and one store per
// slot.  The cotangents are read AFTER eval, per pass: they are not live across the point function (SB2006 Float32 sits at exactly 128 VGPRs at K = 3
// without them), and a second read of a line the first pass brought in is served by the cache.
template <typename S, typename FT, int K, typename C>
__device__ __forceinline__ void vjp_point(const C &c, const VjpArgs<FT, K, S::NOUT, S::NWRT> &a, const FT (&x)[S::NWRT + 1], int64_t i) {
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
        FT g[S::NOUT];
        int gnan = 0;
        const int64_t ic = products_detail::after(i, o[S::NOUT - 1].v);
#pragma unroll
        for (int q = 0; q < S::NOUT; ++q) {
            g[q] = a.cot[q] ? products_detail::ld(a.cot[q], ic) : FT(0);
            gnan |= (int)(g[q] != g[q]);      // bitwise on purpose: no branch
        }
        if (pass == 0) {      // a NaN cotangent poisons the tendencies too (a select: −0 stays −0); the gradients below are NaN through the products
#pragma unroll
            for (int q = 0; q < S::NOUT; ++q)
                if (a.tend[q]) a.tend[q][i] = gnan ? Math<FT>::nan() : S::out(o[q].v, poison);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            FT *const col = a.grad[pass * K + k];
            if (!col) continue;
            // "the first product, then fma" as ONE chain of fma seeded with −0: fma(g, d, −0) is g·d in every bit (x + (−0) = x for every x, ±0 included),
            // so no step has to know whether it is the first.  No cotangent at all: +0.
            FT s = a.ncot ? -FT(0) : FT(0);
#pragma unroll
            for (int q = 0; q < S::NOUT; ++q)
                if (a.cot[q]) s = Math<FT>::fma(g[q], o[q].d[k], s);
            col[i] = S::out(s, poison);
        }
    }
}

#if !defined(CMX_HOST_BUILD)
// The kernels: one point per lane.  `c`, the scheme's constants struct, stays the FIRST kernel argument: front_consts reads it at offset 0 of the kernel-argument segment.
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

template <typename S, typename FT, int BS, typename C>
__global__ __launch_bounds__(BS) void jvp_kernel(const C c, const JvpArgs<FT, S::NOUT, S::NWRT> a, const int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    FT x[S::NWRT + 1], t[S::NWRT];
    if (i < n) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
#pragma unroll
        for (int j = 0; j < S::NWRT; ++j) t[j] = a.tan[j] ? __builtin_nontemporal_load(a.tan[j] + i) : FT(0);
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS while the loads fly (every lane of the workgroup reaches the barrier inside); no-op for Float32
    if (i >= n) return;
    jvp_point<S, FT>(c, a, x, t, i);
}

template <typename S, typename FT, int K, int BS, typename C>
__global__ __launch_bounds__(BS) void vjp_kernel(const C c, const VjpArgs<FT, K, S::NOUT, S::NWRT> a, const int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    FT x[S::NWRT + 1];
    if (i < n) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
    }
    Math<FT>::prepare();
    if (i >= n) return;
    vjp_point<S, FT, K>(c, a, x, i);
}
#endif

}  // namespace cmx
