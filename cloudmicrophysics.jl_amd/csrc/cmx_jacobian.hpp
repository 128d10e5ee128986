// cmx_jacobian.hpp — the forward-mode derivative driver every scheme's entries share (cmx_sb2006_jacobian.hpp, cmx_mp1m_jacobian.hpp), on the device and in the
// host test build (tests/native/derivatives_host.cpp, CMX_HOST_BUILD): the table that maps tangent slots to inputs and, per operation — the Jacobian, J v,
// Jᵀḡ, the linearly implicit tendency (I − Δt J)⁻¹ f, the average tendency over sub-stepped implicit steps — the argument struct, every pass of one point with its stores, and the kernel.  No HIP outside the CMX_HOST_BUILD guards.
//
// A SCHEME is a struct of static members that supplies what differs between two entries:
//   NOUT, NWRT               outputs and differentiated inputs; a point is x[0] = ρ (held fixed) and x[1 … NWRT], the inputs in the order of the entry's wrt enum
//   eval<FT, K>(c, rho, in, o)   the clamps and the point function on Dual<FT, K> (cmx_dual.hpp): o[NOUT] from the seeded in[NWRT].  It reads the constants
//                            through front_consts (cmx_math.hpp) itself, from inside the pass, so that no constant is live across the loop over the passes
//   poison(x), out(v, p)     the entry's NaN rule: p = poison(x) once per point, every stored value and tangent goes through out(·, p)
// (ToyJac of tests/native/derivatives_host.cpp is the smallest one.)
#pragma once
#include <cstdint>
#include <limits>
#include <type_traits>

#include "../../include/cmx.h"
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

// ---- (I − Δt J)⁻¹ f: the tendency of a linearly implicit (Rosenbrock–Euler) step, solved in the pass that holds the tangents in registers -----------------------
// The scheme's outputs are the tendencies f of NOUT of its inputs, the species s = in[S::SPECIES0 … S::SPECIES0 + NOUT − 1] (x[1 + S::SPECIES0 + j]); with
// J = ∂f/∂s at fixed ρ and the other inputs, r = (I − Δt J)⁻¹ f is the tendency of the step s ← s + Δt r.  r and not δ = Δt r: no division, and r = f at Δt = 0.
//   * The tangents are the Jacobian entry's: run-time unit seeds on the species, ⌈NOUT/K⌉ passes, every input made opaque per pass (keep(), see jacobian_point).
//     So J does not depend on K, bit for bit, and is what jacobian_point would store; the primal `tend` is the plain instantiation's bit for bit.
//     The matrix is indexed by constants only and stays in registers.
//   * A = I − Δt J is formed as fma(−Δt, J_ij, δ_ij) and EQUILIBRATED with exact powers of two, taken from the exponent field (pow2_floor), never a rounding
//     multiply: column j by c_j = 2^⌊log2 s_j⌋ of the clamped state (1 for an absent species, s_j ≤ 0) — the unknown becomes the relative change r_j/c_j, and a
//     change of units of a species (kg⁻¹ against kg kg⁻¹: ten orders of magnitude in SB2006) scales row and column of A·diag(c) by the same exact factor —
//     then row i by the inverse of 2^⌊log2 max_j |A_ij c_j|⌋.  Scaling by a power of two commutes with rounding (short of over- and underflow), so it adds no
//     error of its own, and the equilibrated system of a state in other units is the same system.
//   * Gaussian elimination with partial pivoting, fully unrolled: the pivot row moves by compare-and-select swaps (no register array is indexed by a
//     run-time value), ONE reciprocal per pivot (rcp1: the hardware seed with the library's Newton refinement), multipliers and updates as fma.  A multiplier
//     or coefficient that is exactly zero leaves the row untouched in every bit (a select), the sign of a zero included: at Δt = 0 the system is I r = f
//     and r = f in every bit.
//   * ONE step of iterative refinement in the working precision, from the same factors (a residual and a second substitution, no second division).
//     Partial pivoting bounds the backward error in the norm of the row, not component by component, and the relative changes r_j / c_j of a trace species
//     and of a dominant one differ by orders of magnitude: without the step the componentwise backward error ω reached 2e-4 in Float32 (5e-13 in Float64)
//     on the states of tests/implicit_cases.py — a small component wrong in its fourth digit — with it ω ≤ 1 eps (Float32) / 3 eps (Float64) at every
//     state and Δt there (Skeel 1980: one step in fixed precision makes Gaussian elimination componentwise backward stable).  Equilibrating the columns
//     by their maxima instead was worse (ω up to 6e-2), by 2^⌊log2 |f_j|⌋ better (70 eps) but still outside what LAPACK in Float64 rounds to.
// Edge semantics:
//   * A zero pivot — a singular I − Δt J — follows IEEE: rcp1(0) = ±Inf and the point's r is non-finite; that point only, no status, no branch.
//   * An absent species (input ≤ 0) has a zero Jacobian column through the scheme's max0 clamp: its column of A is the unit vector, the solve is regular.
//   * The library's NaN rule through the scheme's poison() / out(): a NaN in any input of the point (the 1-moment Float64 entry: also ρ ≤ 0) gives NaN in
//     every output of that point and in no other.
// All NOUT components of r are computed whatever subset is stored, so a column's bits do not depend on which others are requested.
// Out of scope: carrying T or q_tot in the solve, autograd through the solve, the 2M + P3 scheme.  Sub-stepping inside the kernel and positivity limiting of
// s + Δt r are not this entry's either: they are implicit_average_point's, below.
// Tangents per evaluation of the point function, per float type, for both schemes: tuning numbers (-DCMX_IMPLICIT_K_F32=…, -DCMX_IMPLICIT_K_F64=…; 1, 2 or 4).
// Float32: 1 — the only width inside 128 VGPRs (SB2006 124–127, 1-moment 93–104; K = 2: 148 / 126–142, K = 4: 154 / 159–185, which are faster per call,
// 0.42 / 0.35 against 0.54 ms per 1e7 SB2006 points, and are given up for the four waves per SIMD the other Float32 kernels of the layer keep).  Float64: 4 —
// one pass, 330–336 / 308–398 VGPRs at one wave per SIMD like the Jacobian's own K = 3, 1.05 against 1.58 (K = 1, 255 VGPRs, two waves) and 1.46 ms (K = 2).
// No width spills a VGPR or touches scratch.  The table is DESIGN.md §9; tools/time_implicit.py --fused-only times a build with another K (CMX_LIB).
#ifndef CMX_IMPLICIT_K_F32
#define CMX_IMPLICIT_K_F32 1
#endif
#ifndef CMX_IMPLICIT_K_F64
#define CMX_IMPLICIT_K_F64 4
#endif
template <typename FT> constexpr int kImplicitK = sizeof(FT) == 4 ? CMX_IMPLICIT_K_F32 : CMX_IMPLICIT_K_F64;

namespace implicit_detail {
template <typename FT> struct Pow2;
template <> struct Pow2<float> { using U = uint32_t; static constexpr int MANT = 23, BIAS = 127; };
template <> struct Pow2<double> { using U = uint64_t; static constexpr int MANT = 52, BIAS = 1023; };
// 2^⌊log2 |x|⌋ from the exponent field, kept to [2^(1−BIAS), 2^(BIAS−1)] so that it and its inverse are normal numbers (0 and subnormals give the smallest,
// Inf and NaN the largest)
template <typename FT> __device__ __forceinline__ FT pow2_floor(FT x) {
    using P = Pow2<FT>;
    using U = typename P::U;
    constexpr U lo = (U)1 << P::MANT, hi = (U)(2 * P::BIAS - 1) << P::MANT;
    U u = __builtin_bit_cast(U, x) & ((U)(2 * P::BIAS + 1) << P::MANT);
    u = u < lo ? lo : (u > hi ? hi : u);
    return __builtin_bit_cast(FT, u);
}
// 1/p for p = pow2_floor(·): the exponent field mirrored, exact
template <typename FT> __device__ __forceinline__ FT pow2_inv(FT p) {
    using P = Pow2<FT>;
    using U = typename P::U;
    return __builtin_bit_cast(FT, (U)(((U)(2 * P::BIAS) << P::MANT) - __builtin_bit_cast(U, p)));
}
// 1/d with the IEEE results for d = ±0, ±Inf and NaN: Float64 is the library's rcp (seed, two Newton steps, the seed itself where it is 0 or ±Inf); Float32 the
// hardware seed (1 ulp) with one Newton step and the same fix-up
__device__ __forceinline__ double rcp1(double d) { return Math<double>::rcp(d); }
__device__ __forceinline__ float rcp1(float d) {
    const float r0 = Math<float>::rcp(d);
    const float r = Math<float>::fma(r0, Math<float>::fma(-d, r0, 1.0f), r0);
    return (bool)((int)(r0 == 0.0f) | (int)(__builtin_fabsf(r0) == __builtin_inff())) ? r0 : r;
}
__device__ __forceinline__ float absv(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double absv(double x) { return __builtin_fabs(x); }
template <typename FT> __device__ __forceinline__ void cswap(bool c, FT &a, FT &b) {
    const FT t = c ? b : a;
    b = c ? a : b;
    a = t;
}
// acc − m·v; acc itself, in every bit, where m is exactly zero
template <typename FT> __device__ __forceinline__ FT fnma_nz(FT m, FT v, FT acc) { return m == FT(0) ? acc : Math<FT>::fma(-m, v, acc); }

// P B = L U of an N × N matrix in registers, in place: partial pivoting by compare-and-select swaps, every index a compile-time constant after unrolling.
// Step k exchanges row k with every later row whose entry in column k is larger (sw[k][i]; afterwards row k holds the largest of rows k … N − 1, the first
// one on a tie), in the columns k … N − 1 only: the multipliers of the earlier steps stay where substitute() applies them, between the same exchanges.
// piv[k] = 1 / U_kk, the ONE division of the step; the multipliers take the place of the eliminated entries.
template <typename FT, int N> __device__ __forceinline__ void factor_pivoted(FT (&B)[N][N], bool (&sw)[N][N], FT (&piv)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            sw[k][i] = absv(B[i][k]) > absv(B[k][k]);
#pragma unroll
            for (int j = k; j < N; ++j) cswap(sw[k][i], B[k][j], B[i][j]);
        }
        piv[k] = rcp1(B[k][k]);
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const FT m = B[i][k] * piv[k];
            B[i][k] = m;
#pragma unroll
            for (int j = k + 1; j < N; ++j) B[i][j] = fnma_nz(m, B[k][j], B[i][j]);
        }
    }
}
// g ← (P⁻¹ L U)⁻¹ g from the factors: the exchanges and multipliers of step k in the order factor_pivoted took them, then the back substitution
template <typename FT, int N> __device__ __forceinline__ void substitute(const FT (&LU)[N][N], const bool (&sw)[N][N], const FT (&piv)[N], FT (&g)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int i = k + 1; i < N; ++i) cswap(sw[k][i], g[k], g[i]);
#pragma unroll
        for (int i = k + 1; i < N; ++i) g[i] = fnma_nz(LU[i][k], g[k], g[i]);
    }
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
        FT acc = g[k];
#pragma unroll
        for (int j = k + 1; j < N; ++j) acc = fnma_nz(LU[k][j], g[j], acc);
        g[k] = acc * piv[k];
    }
}
}  // namespace implicit_detail

// `wrt[s]`: the input tangent slot s = pass·K + k is seeded on, S::SPECIES0 + s.  `impl[q]`: the column of r_q, `tend[q]`: the optional primal f_q; both NULL-able.
template <typename FT, int K, int NOUT, int NWRT> struct ImplicitArgs {
    static_assert(NOUT % K == 0, "ImplicitArgs: K divides the number of species");
    const FT *in[NWRT + 1];           // rho, then the differentiated inputs
    FT *impl[NOUT];
    FT *tend[NOUT];
    int32_t wrt[NOUT];
    FT dt;
};

// False if the call has no output column at all.  `implicit` is the caller's table of NOUT members (not NULL itself: the entry checks that), `species0` = S::SPECIES0.
template <typename FT, int K, int NOUT, int NWRT>
inline bool make_implicit_args(ImplicitArgs<FT, K, NOUT, NWRT> &a, const FT *const (&in)[NWRT + 1], int species0, double dt, FT *const *implicit, FT *const *tendencies) {
    a = ImplicitArgs<FT, K, NOUT, NWRT>{};
    for (int j = 0; j < NWRT + 1; ++j) a.in[j] = in[j];
    bool any = false;
    for (int q = 0; q < NOUT; ++q) {
        a.impl[q] = implicit ? implicit[q] : nullptr;
        a.tend[q] = tendencies ? tendencies[q] : nullptr;
        a.wrt[q] = species0 + q;
        any |= a.impl[q] != nullptr || a.tend[q] != nullptr;
    }
    a.dt = (FT)dt;
    return any;
}
// Δt of an implicit entry: finite and ≥ 0
inline bool implicit_dt_ok(double dt) { return dt >= 0.0 && dt < __builtin_inf(); }

// Every pass of one point, the solve and its stores: the body of the kernel's lane and of the host loop.
template <typename S, typename FT, int K, typename C>
__device__ __forceinline__ void implicit_point(const C &c, const ImplicitArgs<FT, K, S::NOUT, S::NWRT> &a, const FT (&x)[S::NWRT + 1], int64_t i) {
    using namespace implicit_detail;
    constexpr int N = S::NOUT;
    static_assert(S::SPECIES0 >= 0 && S::SPECIES0 + N <= S::NWRT, "implicit_point: the species block lies inside the differentiated inputs");
    FT B[N][N] = {}, g[N] = {};
#pragma unroll 1
    for (int pass = 0; pass < N / K; ++pass) {
        Dual<FT, K> in[S::NWRT], o[N];
#pragma unroll
        for (int j = 0; j < S::NWRT; ++j) {
            in[j].v = keep(x[j + 1]);
#pragma unroll
            for (int k = 0; k < K; ++k) in[j].d[k] = a.wrt[pass * K + k] == j ? FT(1) : FT(0);
        }
        S::template eval<FT, K>(c, keep(x[0]), in, o);
        // f from the LAST pass (every pass's primal is the same, bit for bit): not alive across the point function
        if (pass == N / K - 1) {
#pragma unroll
            for (int q = 0; q < N; ++q) g[q] = o[q].v;
        }
        // column pass·K + k of A = I − Δt J.  The loop over the passes stays a loop (unrolled, the passes interleave and every intermediate of two point
        // functions is alive at once), so the column is placed by selects over constant indices, not by an index
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int s = 0; s < N; ++s) {
                const bool here = s == pass * K + k;
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    const FT v = Math<FT>::fma(-a.dt, o[q].d[k], q == s ? FT(1) : FT(0));
                    B[q][s] = here ? v : B[q][s];
                }
            }
        }
    }
    const auto poison = S::poison(x);
#pragma unroll
    for (int q = 0; q < N; ++q)
        if (a.tend[q]) a.tend[q][i] = S::out(g[q], poison);
    FT cs[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const FT s = x[1 + S::SPECIES0 + j];
        cs[j] = pow2_floor(s > FT(0) ? s : FT(1));
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
        FT m = FT(0);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            B[q][j] *= cs[j];
            m = Math<FT>::max(m, absv(B[q][j]));
        }
        const FT rs = pow2_inv(pow2_floor(m));
#pragma unroll
        for (int j = 0; j < N; ++j) B[q][j] *= rs;
        g[q] *= rs;
    }
    // z from the factors, then ONE step of iterative refinement in working precision: ρ = g − B z against the unfactored B, the correction from the same factors
    FT LU[N][N], piv[N], res[N], z[N];
    bool sw[N][N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        z[q] = g[q];
#pragma unroll
        for (int j = 0; j < N; ++j) LU[q][j] = B[q][j];
    }
    factor_pivoted<FT, N>(LU, sw, piv);
    substitute<FT, N>(LU, sw, piv, z);
#pragma unroll
    for (int q = 0; q < N; ++q) {
        res[q] = g[q];
#pragma unroll
        for (int j = 0; j < N; ++j) res[q] = fnma_nz(B[q][j], z[j], res[q]);
    }
    substitute<FT, N>(LU, sw, piv, res);
#pragma unroll
    for (int q = 0; q < N; ++q) g[q] = res[q] == FT(0) ? z[q] : z[q] + res[q];      // a zero correction leaves z as it is, the sign of a zero included
#pragma unroll
    for (int q = 0; q < N; ++q)
        if (a.impl[q]) a.impl[q][i] = S::out(g[q] * cs[q], poison);
}

// implicit_point without its stores: r = (I − Δt J)⁻¹ f of the point x, before the scheme's out() — the passes, the equilibration, the factorisation and the
// refinement step of implicit_point, operation for operation, so that r is implicit_point's in every bit (tests/test_implicit_average_host.py and
// tests/test_implicit_average_gpu.py compare them through the recipe).  `wrt`: the slot table of ImplicitArgs.  The body of a substep of
// implicit_average_point.  implicit_point does NOT call it: as its caller it compiled to other Float64 code (SB2006 334 → 338–340 VGPRs, the 1-moment default
// instantiation 10 → 12 spilled SGPRs; two forms tried, with the primal's stores as a callback), and the existing entries keep the parent's code.
template <typename S, typename FT, int K, typename C>
__device__ __forceinline__ void implicit_solve(const C &c, const int32_t (&wrt)[S::NOUT], FT dt, const FT (&x)[S::NWRT + 1], FT (&r)[S::NOUT]) {
    using namespace implicit_detail;
    constexpr int N = S::NOUT;
    static_assert(S::SPECIES0 >= 0 && S::SPECIES0 + N <= S::NWRT, "implicit_solve: the species block lies inside the differentiated inputs");
    FT B[N][N] = {}, g[N] = {};
#pragma unroll 1
    for (int pass = 0; pass < N / K; ++pass) {
        Dual<FT, K> in[S::NWRT], o[N];
#pragma unroll
        for (int j = 0; j < S::NWRT; ++j) {
            in[j].v = keep(x[j + 1]);
#pragma unroll
            for (int k = 0; k < K; ++k) in[j].d[k] = wrt[pass * K + k] == j ? FT(1) : FT(0);
        }
        S::template eval<FT, K>(c, keep(x[0]), in, o);
        // f from EVERY pass (every pass's primal is the same, bit for bit), so from the last: overwritten per pass, f is not alive across the point function
        // — nor are four registers that wait for the last pass, as with implicit_point's `if (pass == N / K − 1)`
#pragma unroll
        for (int q = 0; q < N; ++q) g[q] = o[q].v;
        // column pass·K + k of A = I − Δt J.  The loop over the passes stays a loop (unrolled, the passes interleave and every intermediate of two point
        // functions is alive at once), so the column is placed by selects over constant indices, not by an index
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int s = 0; s < N; ++s) {
                const bool here = s == pass * K + k;
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    const FT v = Math<FT>::fma(-dt, o[q].d[k], q == s ? FT(1) : FT(0));
                    B[q][s] = here ? v : B[q][s];
                }
            }
        }
    }
    FT cs[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const FT s = x[1 + S::SPECIES0 + j];
        cs[j] = pow2_floor(s > FT(0) ? s : FT(1));
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
        FT m = FT(0);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            B[q][j] *= cs[j];
            m = Math<FT>::max(m, absv(B[q][j]));
        }
        const FT rs = pow2_inv(pow2_floor(m));
#pragma unroll
        for (int j = 0; j < N; ++j) B[q][j] *= rs;
        g[q] *= rs;
    }
    // z from the factors, then ONE step of iterative refinement in working precision: ρ = g − B z against the unfactored B, the correction from the same factors
    FT LU[N][N], piv[N], res[N], z[N];
    bool sw[N][N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        z[q] = g[q];
#pragma unroll
        for (int j = 0; j < N; ++j) LU[q][j] = B[q][j];
    }
    factor_pivoted<FT, N>(LU, sw, piv);
    substitute<FT, N>(LU, sw, piv, z);
#pragma unroll
    for (int q = 0; q < N; ++q) {
        res[q] = g[q];
#pragma unroll
        for (int j = 0; j < N; ++j) res[q] = fnma_nz(B[q][j], z[j], res[q]);
    }
    substitute<FT, N>(LU, sw, piv, res);
#pragma unroll
    for (int q = 0; q < N; ++q) g[q] = res[q] == FT(0) ? z[q] : z[q] + res[q];      // a zero correction leaves z as it is, the sign of a zero included
#pragma unroll
    for (int q = 0; q < N; ++q) r[q] = g[q] * cs[q];
}

// ---- The average tendency over Δt from nsub linearly implicit substeps, the substep loop inside the kernel (include/cmx.h §(19)) ----------------------------------
// What a host model calls per time step: nsub steps s ← s + h r of the solve above with h = Δt/nsub, the temperature following the latent heating of every
// substep (ρ and q_tot fixed), and (s_end − s_start)/Δt as the result.  The definition is normative, bit for bit: every product and sum below is one IEEE
// operation of the float type (no fma), the selects are selects (a NaN stays a NaN):
//     repeat nsub times:
//         r    = out(implicit_solve(ρ, T, q_tot, s; Δt = h), poison(ρ, T, q_tot, s))      — the implicit entry's result at the current state
//         sn_j = s_j + r_j·h
//         CMX_STEP_NONNEGATIVE:  lo_j = s_j < 0 ? s_j : 0;  sn_j = sn_j < lo_j ? lo_j : sn_j
//         d_j  = (sn_j − s_j)·inv_h
//         T    = T + S::heating(Lv, Ls, d)·h
//         s    = sn
//     average_j = (s_j − s0_j)·inv_dt
// The limiter: a species never ends a substep below 0, one that was negative already never below where it started.  Without it the Rosenbrock–Euler step
// leaves a species negative at 17 % (SB2006) and 58 % (1-moment) of the states of tests/implicit_cases.py at Δt = 30 s, nsub = 1; it does not touch the
// first order of the scheme.  A NaN in an input makes the first r NaN in all components (poison), and so all four averages of that point and of no other;
// a singular substep solve makes that point non-finite.
// Registers: alive across the point function are the point x (as in implicit_point), s0 and the uniform loop counter; nothing is read again from memory.
// Reading ρ, q_tot per substep and s0 after the loop instead (non-temporal, behind an opaque index) saved 4–6 VGPRs that no instantiation needed and cost a
// memory latency that the one Float64 wave per SIMD cannot hide: 1.32 against 1.06 ms of ONE implicit call at nsub = 1 and 1e7 SB2006 Float64 points.  What
// made room is implicit_solve taking f from every pass: SB2006 Float32 129–132 → 101–104 VGPRs.  All of a lane's reads come before its writes: `average`
// may alias the species columns.
// K per float type: -DCMX_IMPLICIT_AVG_K_F32=…, -DCMX_IMPLICIT_AVG_K_F64=… (1, 2 or 4), by default the implicit entry's; the register table is DESIGN.md §9.
#ifndef CMX_IMPLICIT_AVG_K_F32
#define CMX_IMPLICIT_AVG_K_F32 CMX_IMPLICIT_K_F32
#endif
#ifndef CMX_IMPLICIT_AVG_K_F64
#define CMX_IMPLICIT_AVG_K_F64 CMX_IMPLICIT_K_F64
#endif
template <typename FT> constexpr int kImplicitAvgK = sizeof(FT) == 4 ? CMX_IMPLICIT_AVG_K_F32 : CMX_IMPLICIT_AVG_K_F64;

// `avg[q]`: the column of average_q (NULL-able).  h = Δt/nsub and the reciprocals as make_mp1m_lin_args (cmx_mp1m.hpp) forms them; Lv = LH_v0/cp_d, Ls = LH_s0/cp_d.
template <typename FT, int K, int NOUT, int NWRT> struct ImplicitAverageArgs {
    static_assert(NOUT % K == 0, "ImplicitAverageArgs: K divides the number of species");
    const FT *in[NWRT + 1];           // rho, then the differentiated inputs
    FT *avg[NOUT];
    int32_t wrt[NOUT];
    int32_t nsub;
    uint32_t step_flags;
    FT h, inv_h, inv_dt, Lv, Ls;
};

// Δt, nsub and the step flags of an average entry: Δt finite and > 0, 1 ≤ nsub ≤ CMX_IMPLICIT_AVERAGE_MAX_NSUB, no unknown flag bit, and h and 1/Δt finite
// positive normal numbers of the float type (then 1/h is one too)
template <typename FT> inline bool implicit_average_step_ok(double dt, int32_t nsub, uint32_t step_flags) {
    if (!(dt > 0.0 && dt < __builtin_inf())) return false;
    if (nsub < 1 || nsub > CMX_IMPLICIT_AVERAGE_MAX_NSUB) return false;
    if (step_flags & ~(uint32_t)CMX_STEP_NONNEGATIVE) return false;
    const FT dt_f = (FT)dt, h = dt_f / (FT)nsub, inv_dt = FT(1) / dt_f;
    const auto normal = [](FT v) { return v >= std::numeric_limits<FT>::min() && v <= std::numeric_limits<FT>::max(); };
    return normal(h) && normal(inv_dt);
}

// False if the call has no output column at all.  `average` is the caller's table of NOUT members (not NULL itself: the entry checks that, and
// implicit_average_step_ok before this).  LH_v0, LH_s0, cp_d: the thermodynamics struct's fields.
template <typename FT, int K, int NOUT, int NWRT>
inline bool make_implicit_average_args(ImplicitAverageArgs<FT, K, NOUT, NWRT> &a, const FT *const (&in)[NWRT + 1], int species0, double dt, int32_t nsub,
                                       uint32_t step_flags, FT LH_v0, FT LH_s0, FT cp_d, FT *const *average) {
    a = ImplicitAverageArgs<FT, K, NOUT, NWRT>{};
    for (int j = 0; j < NWRT + 1; ++j) a.in[j] = in[j];
    bool any = false;
    for (int q = 0; q < NOUT; ++q) {
        a.avg[q] = average ? average[q] : nullptr;
        a.wrt[q] = species0 + q;
        any |= a.avg[q] != nullptr;
    }
    const FT dt_f = (FT)dt;
    a.nsub = nsub;
    a.step_flags = step_flags;
    a.h = dt_f / (FT)nsub;
    a.inv_h = FT(1) / a.h;
    a.inv_dt = FT(1) / dt_f;
    a.Lv = LH_v0 / cp_d;
    a.Ls = LH_s0 / cp_d;
    return any;
}

// The substeps of one point, the averages returned in registers: the loop of implicit_average_kernel, of implicit_sedimentation_step_kernel
// (cmx_column_implicit_step.hip) and of the host loop.  (implicit_average_column_kernel, cmx_column_implicit_average.hip, keeps a copy: the call was measured
// slower there.  A change here is a change there.)  x: the point as the kernel read it; the species and T (x[1 + S::TEMP], if the scheme has one) advance in it.
// A: ImplicitAverageArgs<FT, K, S::NOUT, S::NWRT>, or a view with its members wrt, nsub, step_flags, h, inv_h, inv_dt, Lv, Ls (the ensemble form of the column
// step, cmx_column_implicit_step_ensemble.hip, whose Lv and Ls are a member's).
template <typename S, typename FT, int K, typename C, typename A>
__device__ __forceinline__ void implicit_average_substeps(const C &c, const A &a, FT (&x)[S::NWRT + 1], FT (&avg)[S::NOUT]) {
    constexpr int N = S::NOUT, S0 = 1 + S::SPECIES0;
    const bool limit = a.step_flags & CMX_STEP_NONNEGATIVE;
    FT s0[N];
#pragma unroll
    for (int q = 0; q < N; ++q) s0[q] = x[S0 + q];
#pragma unroll 1
    for (int32_t sub = 0; sub < a.nsub; ++sub) {
        FT r[N], d[N];
        implicit_solve<S, FT, K>(c, a.wrt, a.h, x, r);
        const auto poison = S::poison(x);
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const FT s = x[S0 + q];
            FT sn = s + S::out(r[q], poison) * a.h;
            if (limit) {
                const FT lo = s < FT(0) ? s : FT(0);
                sn = sn < lo ? lo : sn;
            }
            d[q] = (sn - s) * a.inv_h;
            x[S0 + q] = sn;
        }
        if constexpr (S::TEMP >= 0) x[1 + S::TEMP] = x[1 + S::TEMP] + S::heating(a.Lv, a.Ls, d) * a.h;
    }
#pragma unroll
    for (int q = 0; q < N; ++q) avg[q] = (x[S0 + q] - s0[q]) * a.inv_dt;
}

// The substeps and their stores: the body of implicit_average_kernel's lane
template <typename S, typename FT, int K, typename C>
__device__ __forceinline__ void implicit_average_point(const C &c, const ImplicitAverageArgs<FT, K, S::NOUT, S::NWRT> &a, FT (&x)[S::NWRT + 1], int64_t i) {
    FT avg[S::NOUT];
    implicit_average_substeps<S, FT, K>(c, a, x, avg);
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q)
        if (a.avg[q]) a.avg[q][i] = avg[q];
}

// ---- ∂/∂θ: the derivatives with respect to the scheme's PARAMETERS (include/cmx.h §(22)) ------------------------------------------------------------------------
// The roles are exchanged: the state enters as constants — Dual(x), every tangent a structural zero that costs nothing — and the CONSTANTS are the duals: the
// scheme's constants struct on Dual<FT, KP>, whose tangent slot k holds ċ = Dc(θ)[δθ⁽ᵏ⁾] of direction k, formed on the host in exact forward mode
// (cmx_param_tangent.hpp).  The point function is the one every other entry runs; all constant tangents are run-time values, so nothing about them folds.
//   * KP directions per evaluation, a tuning number per float type (-DCMX_PARAM_K_F32=…, -DCMX_PARAM_K_F64=…): 4 / 2.  A launch costs about the same whatever
//     share of its slots is in use (measured, one MI355X, 1e7 points, ms per launch of the SB2006 gradient kernel — Float32 KP = 1, 2, 4: 0.18, 0.36, 0.36;
//     Float64 KP = 1, 2: 0.58, 0.73), so a call takes wide launches while at least kParamWideMin directions remain (3 / 2: where the wide launch is cheaper than
//     single ones) and single-direction launches for the rest.  (Timed on the SB2006 gradient kernel only; the jvp kernels and the 1-moment scheme take the same numbers.)  Each tangent slot is computed by the same operations whatever KP is and whatever the other slots
//     hold, so a column's bits do not depend on KP, on the other directions of the call or on how the call was split.  Registers: HISTORY.md.
//   * The value parts are the plain instantiation's bit for bit, like every dual evaluation (cmx_dual.hpp).
//   * The NaN rule is the scheme's: every stored value goes through out(·, poison(x)).
#ifndef CMX_PARAM_K_F32
#define CMX_PARAM_K_F32 4
#endif
#ifndef CMX_PARAM_K_F64
#define CMX_PARAM_K_F64 2
#endif
template <typename FT> constexpr int kParamK = sizeof(FT) == 4 ? CMX_PARAM_K_F32 : CMX_PARAM_K_F64;
template <typename FT> constexpr int kParamWideMin = sizeof(FT) == 4 ? 3 : 2;
// The launches of a call: f(std::integral_constant<int, KP>{}, d0) for the directions d0 … d0 + KP − 1, wide (kParamK) while at least kParamWideMin remain,
// then one direction at a time.
template <typename FT, typename F> inline void for_each_param_launch(int ndir, F &&f) {
    for (int d0 = 0; d0 < ndir;) {
        if (kParamK<FT> > 1 && ndir - d0 >= kParamWideMin<FT>) {
            f(std::integral_constant<int, kParamK<FT>>{}, d0);
            d0 += kParamK<FT>;
        } else {
            f(std::integral_constant<int, 1>{}, d0);
            d0 += 1;
        }
    }
}

// (shared by the column steps' parameter derivatives, cmx_sb2006_column_param.hpp and cmx_mp1m_column_param.hpp)
// f(std::integral_constant<int, 0>{}) … f(std::integral_constant<int, N − 1>{}): the loops over the flux slots with the slot a compile-time constant.  With KP
// tangents inside, `#pragma unroll` alone left the slot loop of the cloud instantiations rolled, and Av[flux_out(s)] became a run-time index into a
// stack copy of the point (77 scratch instructions at KP = 4).
template <int N, typename F> __device__ __forceinline__ void for_each_slot(F &&f) {
    if constexpr (N > 0) {
        for_each_slot<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// The launches of a call: f(std::integral_constant<int, K>{}, d0) for the directions d0 … d0 + K − 1 — KW at a time while at least min(KW, 2) remain, then
// one at a time.
template <int KW, typename F> inline void for_each_column_param_launch(int ndir, F &&f) {
    for (int d0 = 0; d0 < ndir;) {
        if (KW > 1 && ndir - d0 >= 2) {
            f(std::integral_constant<int, KW>{}, d0);
            d0 += KW;
        } else {
            f(std::integral_constant<int, 1>{}, d0);
            d0 += 1;
        }
    }
}

// `jvp[k][q]`: the column of Σ_p ∂out_q/∂θ_p·δθ_p of the direction in tangent slot k (NULL: not wanted, or an idle slot).  `tend`: the optional primal columns.
template <typename FT, int KP, int NOUT, int NWRT> struct ParamJvpArgs {
    const FT *in[NWRT + 1];           // rho, then the other inputs
    FT *tend[NOUT];
    FT *jvp[KP][NOUT];
};

// the scheme on the dual constants `cd` at the point x
template <typename S, typename FT, int KP, typename CD>
__device__ __forceinline__ void param_eval(const CD &cd, const FT (&x)[S::NWRT + 1], Dual<FT, KP> (&o)[S::NOUT]) {
    Dual<FT, KP> in[S::NWRT];
#pragma unroll
    for (int j = 0; j < S::NWRT; ++j) in[j] = Dual<FT, KP>(x[j + 1]);
    S::template eval<FT, KP>(cd, x[0], in, o);
}

template <typename S, typename FT, int KP, typename CD>
__device__ __forceinline__ void param_jvp_point(const CD &cd, const ParamJvpArgs<FT, KP, S::NOUT, S::NWRT> &a, const FT (&x)[S::NWRT + 1], int64_t i) {
    const auto poison = S::poison(x);
    Dual<FT, KP> o[S::NOUT];
    param_eval<S, FT, KP>(cd, x, o);
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q)
        if (a.tend[q]) a.tend[q][i] = S::out(o[q].v, poison);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
#pragma unroll
        for (int q = 0; q < S::NOUT; ++q) {
            FT *const col = a.jvp[k][q];
            if (col) col[i] = S::out(o[q].d[k], poison);
        }
    }
}

// The gradient is a REDUCTION over the points: grad[d] = Σ_i Σ_q ḡ_q,i·(∂out_q/∂θ·δθ⁽ᵈ⁾)_i.  Per point the Σ_q is vjp_point's chain of fma over the non-NULL
// cotangents (seeded with −0; no cotangent at all: +0), read after eval; it goes through out(·, poison), is widened to double and added to the lane's
// accumulator of the slot.  A NaN in the state or in a cotangent of a point makes the sum NaN (IEEE) and that point's tendencies NaN.
template <typename FT, int NOUT, int NWRT> struct ParamVjpArgs {
    const FT *in[NWRT + 1];
    const FT *cot[NOUT];
    FT *tend[NOUT];
    int32_t ncot;                     // the non-NULL members of cot
};

template <typename S, typename FT, int KP, typename CD>
__device__ __forceinline__ void param_vjp_point(const CD &cd, const ParamVjpArgs<FT, S::NOUT, S::NWRT> &a, const FT (&x)[S::NWRT + 1], int64_t i, double (&acc)[KP]) {
    const auto poison = S::poison(x);
    Dual<FT, KP> o[S::NOUT];
    param_eval<S, FT, KP>(cd, x, o);
    FT g[S::NOUT];
    int gnan = 0;
    const int64_t ic = products_detail::after(i, o[S::NOUT - 1].v);
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q) {
        g[q] = a.cot[q] ? products_detail::ld(a.cot[q], ic) : FT(0);
        gnan |= (int)(g[q] != g[q]);      // bitwise on purpose: no branch
    }
#pragma unroll
    for (int q = 0; q < S::NOUT; ++q)
        if (a.tend[q]) a.tend[q][i] = gnan ? Math<FT>::nan() : S::out(o[q].v, poison);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        FT s = a.ncot ? -FT(0) : FT(0);
#pragma unroll
        for (int q = 0; q < S::NOUT; ++q)
            if (a.cot[q]) s = Math<FT>::fma(g[q], o[q].d[k], s);
        acc[k] += (double)S::out(s, poison);
    }
}

// The decomposition of the reduction, a function of n alone (not of the device): CMX_PARAM_VJP_PARTIALS workgroups of `bs` lanes, workgroup b owns the
// contiguous chunk [b·chunk, (b + 1)·chunk), chunk = n split that many ways and rounded up to a multiple of bs; lane t of it takes the points
// b·chunk + t, + bs, … in index order.
inline int64_t param_vjp_chunk(int64_t n, int64_t bs) {
    const int64_t c = (n + CMX_PARAM_VJP_PARTIALS - 1) / CMX_PARAM_VJP_PARTIALS;
    return (c + bs - 1) / bs * bs;
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

template <typename S, typename FT, int K, int BS, typename C>
__global__ __launch_bounds__(BS) void implicit_kernel(const C c, const ImplicitArgs<FT, K, S::NOUT, S::NWRT> a, const int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    FT x[S::NWRT + 1];
    if (i < n) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
    }
    Math<FT>::prepare();
    if (i >= n) return;
    implicit_point<S, FT, K>(c, a, x, i);
}

template <typename S, typename FT, int K, int BS, typename C>
__global__ __launch_bounds__(BS) void implicit_average_kernel(const C c, const ImplicitAverageArgs<FT, K, S::NOUT, S::NWRT> a, const int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    FT x[S::NWRT + 1];
    if (i < n) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
    }
    Math<FT>::prepare();
    if (i >= n) return;
    implicit_average_point<S, FT, K>(c, a, x, i);
}

// ∂/∂θ·δθ: the constants struct `c` holds duals — still the first kernel argument, no copy and no allocation on the device
template <typename S, typename FT, int KP, int BS, typename CD>
__global__ __launch_bounds__(BS) void param_jvp_kernel(const CD c, const ParamJvpArgs<FT, KP, S::NOUT, S::NWRT> a, const int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    FT x[S::NWRT + 1];
    if (i < n) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
    }
    Math<FT>::prepare();
    if (i >= n) return;
    param_jvp_point<S, FT, KP>(c, a, x, i);
}

// The end of stage 1 of the gradient, shared by every kernel that feeds the reduction (param_vjp_kernel below; column_param_vjp_kernel,
// cmx_column_products.hpp): the lane's accumulators, then the 64 lanes of a wave in a fixed shuffle tree, then the waves left to right →
// ws[k·CMX_PARAM_VJP_PARTIALS + b].  Every lane of the workgroup calls it.
template <int KP, int BS> __device__ __forceinline__ void param_vjp_reduce(const double (&acc)[KP], const int32_t nlive, double *__restrict__ ws) {
    static_assert(BS % 64 == 0 && KP <= BS, "whole waves");
    __shared__ double part[KP][BS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        double t = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
        if (lane == 0) part[k][wave] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < nlive) {      // nlive ≤ KP: the slots of the launch that hold a direction; the workspace has no room for the idle ones
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < BS / 64; ++w) t += part[threadIdx.x][w];
        ws[(int64_t)threadIdx.x * CMX_PARAM_VJP_PARTIALS + blockIdx.x] = t;
    }
}

// Stage 1 of the gradient (param_vjp_chunk has the decomposition): the lane's accumulators, then param_vjp_reduce.  No floating-point atomics: the result is
// a pure function of the inputs and n, bit-identical from run to run.
template <typename S, typename FT, int KP, int BS, typename CD>
__global__ __launch_bounds__(BS) void param_vjp_kernel(const CD c, const ParamVjpArgs<FT, S::NOUT, S::NWRT> a, const int64_t n, const int64_t chunk,
                                                       const int32_t nlive, double *__restrict__ ws) {
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    Math<FT>::prepare();
    double acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int64_t i = lo + threadIdx.x; i < hi; i += BS) {
        FT x[S::NWRT + 1];
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
        param_vjp_point<S, FT, KP>(c, a, x, i, acc);
    }
    param_vjp_reduce<KP, BS>(acc, nlive, ws);
}

// Stage 2: one workgroup per direction; lane t adds the partials 4t … 4t + 3 left to right, then the same tree → grad[d].
template <int BS> __global__ __launch_bounds__(BS) void param_vjp_finish_kernel(const double *__restrict__ ws, double *__restrict__ grad) {
    static_assert(CMX_PARAM_VJP_PARTIALS == 4 * BS && BS % 64 == 0, "stage 2 gives each lane four partials");
    const double *p = ws + (int64_t)blockIdx.x * CMX_PARAM_VJP_PARTIALS + 4 * threadIdx.x;
    double t = ((p[0] + p[1]) + p[2]) + p[3];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    __shared__ double part[BS / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < BS / 64; ++w) s += part[w];
        grad[blockIdx.x] = s;
    }
}
#endif

}  // namespace cmx
