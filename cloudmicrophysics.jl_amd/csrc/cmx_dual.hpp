// cmx_dual.hpp — forward-mode dual numbers as a VALUE TYPE of the point functions (cmx_math.hpp): Dual<FT, K> carries a value and K tangents, and
// Math<Dual<FT, K>> provides every operation a point function uses, so a Jacobian is one more instantiation of the point function — next to float, double,
// the packed pair f32x2, the counting type of tools/census and the host build — and not a second implementation of the physics.  The reference computes its
// derivatives the same way (ForwardDiff.Dual through the rate functions, test/ad_compat_tests.jl).
//
// Rules:
//   * VALUE.  The value part is computed by exactly the operations of the FT instantiation, in the same order; the library is built with -ffp-contract=off, so
//     the primal of a dual evaluation is bit-identical to the plain evaluation (the reference's f(x) == v₀).
//   * TANGENTS follow the analytic rule of the mathematical function and reuse the value already computed: d exp2(x) = ln2·exp2(x)·dx costs one multiply per
//     tangent, d rcp(x) = −rcp(x)²·dx, d rsqrt(x) = −½·rsqrt(x)³·dx; d log2(x) = dx/(x ln2) issues ONE reciprocal of the argument for all K tangents.
//   * BRANCHING operations — min, max, clampv, clamp_ordered, max0 and the C++ conditional — carry the tangents of the operand whose VALUE is returned
//     (ForwardDiff's rule); compares act on the value.  A gate of a point function is a select `gate ? 0 : rate` of whole duals, so a gated-off rate contributes
//     zero tangents and a non-finite tangent of the side that is not selected is discarded with it.
//   * STRUCTURAL ZEROS.  A tangent that is the literal 0 at compile time — a constant FT(c), a kernel constant, an input that is not differentiated (ρ) and
//     everything computed from those alone — is not multiplied out: 0·x is not 0 in IEEE arithmetic (x may be Inf) and no optimiser may fold it, so the rules
//     below test __builtin_constant_p on each tangent, which the compiler resolves after inlining.  ρ^(−1/2), √(ρ0/ρ) and the like then cost what they cost in
//     the plain instantiation.  A tangent that is zero at RUN time (a seed that is not set) is computed like any other.
//     This is an optimisation the COMPILER decides: where it cannot prove a tangent constant (another compiler, -O0) the full rule a·x + b·y runs instead
//     of a·x, so the tangent EXPRESSIONS of two builds — the host test build and the device build, say — may differ in such terms (by the sign of a zero, or
//     a NaN from 0·Inf behind a gate, which the select discards); the value parts never do, and within one build every tangent slot takes the same path,
//     since the seeds are run-time values.  A compile-time tag would need the point functions to spell their constants differently from `FT(c)`.
#pragma once
#include "cmx_math.hpp"

namespace cmx {

template <typename FT, int K> struct Dual;

namespace dual_detail {
// "this tangent is the literal zero": decided at compile time, after inlining (false where the compiler cannot tell)
template <typename FT> __device__ __forceinline__ bool cz(FT x) { return __builtin_constant_p(x) && x == FT(0); }
// a·x + b·y of tangents with the structural zeros left out
template <typename FT> __device__ __forceinline__ FT lin2(FT a, FT x, FT b, FT y) {
    const bool zx = cz(x), zy = cz(y);
    if (zx && zy) return FT(0);
    if (zy) return a * x;
    if (zx) return b * y;
    return Math<FT>::fma(a, x, b * y);
}
template <typename FT> __device__ __forceinline__ FT scale(FT a, FT x) { return cz(x) ? FT(0) : a * x; }
template <typename FT> __device__ __forceinline__ FT add(FT x, FT y) { return cz(x) ? y : (cz(y) ? x : x + y); }
template <typename FT> __device__ __forceinline__ FT sub(FT x, FT y) { return cz(y) ? x : (cz(x) ? -y : x - y); }
}  // namespace dual_detail

template <typename FT, int K> struct Dual {
    static_assert(std::is_same<FT, float>::value || std::is_same<FT, double>::value, "Dual<FT, K>: FT is float or double");
    static_assert(K >= 1, "Dual<FT, K>: at least one tangent");
    FT v;
    FT d[K];

    Dual() = default;
    // a constant: every tangent is the literal zero
    template <typename A, typename = std::enable_if_t<std::is_arithmetic<A>::value>> __device__ __forceinline__ Dual(A x) : v((FT)x) {
#pragma unroll
        for (int k = 0; k < K; ++k) d[k] = FT(0);
    }

#define CMX_DUAL_FOR for (int k = 0; k < K; ++k)
    friend __device__ __forceinline__ Dual operator-(const Dual &a) {
        Dual r; r.v = -a.v;
#pragma unroll
        CMX_DUAL_FOR r.d[k] = dual_detail::cz(a.d[k]) ? FT(0) : -a.d[k];
        return r;
    }
    friend __device__ __forceinline__ Dual operator+(const Dual &a, const Dual &b) {
        Dual r; r.v = a.v + b.v;
#pragma unroll
        CMX_DUAL_FOR r.d[k] = dual_detail::add(a.d[k], b.d[k]);
        return r;
    }
    friend __device__ __forceinline__ Dual operator+(const Dual &a, FT b) { Dual r = a; r.v = a.v + b; return r; }
    friend __device__ __forceinline__ Dual operator+(FT a, const Dual &b) { Dual r = b; r.v = a + b.v; return r; }
    friend __device__ __forceinline__ Dual operator-(const Dual &a, const Dual &b) {
        Dual r; r.v = a.v - b.v;
#pragma unroll
        CMX_DUAL_FOR r.d[k] = dual_detail::sub(a.d[k], b.d[k]);
        return r;
    }
    friend __device__ __forceinline__ Dual operator-(const Dual &a, FT b) { Dual r = a; r.v = a.v - b; return r; }
    friend __device__ __forceinline__ Dual operator-(FT a, const Dual &b) { Dual r = -b; r.v = a - b.v; return r; }
    friend __device__ __forceinline__ Dual operator*(const Dual &a, const Dual &b) {
        Dual r; r.v = a.v * b.v;
#pragma unroll
        CMX_DUAL_FOR r.d[k] = dual_detail::lin2(b.v, a.d[k], a.v, b.d[k]);
        return r;
    }
    friend __device__ __forceinline__ Dual operator*(const Dual &a, FT b) {
        Dual r; r.v = a.v * b;
#pragma unroll
        CMX_DUAL_FOR r.d[k] = dual_detail::scale(b, a.d[k]);
        return r;
    }
    friend __device__ __forceinline__ Dual operator*(FT a, const Dual &b) {
        Dual r; r.v = a * b.v;
#pragma unroll
        CMX_DUAL_FOR r.d[k] = dual_detail::scale(a, b.d[k]);
        return r;
    }
    __device__ __forceinline__ Dual &operator+=(const Dual &b) { return *this = *this + b; }

    // compares act on the value
#define CMX_DUAL_CMP(op)                                                                                          \
    friend __device__ __forceinline__ bool operator op(const Dual &a, const Dual &b) { return a.v op b.v; }       \
    friend __device__ __forceinline__ bool operator op(const Dual &a, FT b) { return a.v op b; }                  \
    friend __device__ __forceinline__ bool operator op(FT a, const Dual &b) { return a op b.v; }
    CMX_DUAL_CMP(<) CMX_DUAL_CMP(<=) CMX_DUAL_CMP(>) CMX_DUAL_CMP(>=) CMX_DUAL_CMP(==) CMX_DUAL_CMP(!=)
#undef CMX_DUAL_CMP
};

namespace dual_detail {
// value and tangent of an argument that is a dual or a scalar (a scalar's tangent is the literal zero)
template <typename FT, int K> __device__ __forceinline__ FT val(const Dual<FT, K> &x) { return x.v; }
template <typename FT, int K> __device__ __forceinline__ FT tan(const Dual<FT, K> &x, int k) { return x.d[k]; }
template <typename A, typename = std::enable_if_t<std::is_arithmetic<A>::value>> __device__ __forceinline__ A val(A x) { return x; }
template <typename A, typename = std::enable_if_t<std::is_arithmetic<A>::value>> __device__ __forceinline__ A tan(A, int) { return A(0); }
}  // namespace dual_detail

template <typename FT, int K> struct Math<Dual<FT, K>> {
    using D = Dual<FT, K>;
    using MS = Math<FT>;
    using Scalar = FT;
    using Mask = bool;
    static constexpr bool IS_F64 = MS::IS_F64;
    static constexpr FT eps() { return MS::eps(); }
    static constexpr FT eps_1m() { return MS::eps_1m(); }
    static __device__ __forceinline__ void prepare() { MS::prepare(); }
    static __device__ __forceinline__ D nan() { return D(MS::nan()); }

    // y = f(x.v) already computed, f'(x.v) = g: every tangent is g·dx
    static __device__ __forceinline__ D chain(FT y, FT g, const D &x) {
        D r; r.v = y;
#pragma unroll
        CMX_DUAL_FOR r.d[k] = dual_detail::scale(g, x.d[k]);
        return r;
    }
    static __device__ __forceinline__ D exp2_rule(FT e, const D &x) { return chain(e, FT(0.6931471805599453) * e, x); }
    static __device__ __forceinline__ D exp2(const D &x) { return exp2_rule(MS::exp2(x.v), x); }
    static __device__ __forceinline__ D exp2_fin(const D &x) { return exp2_rule(MS::exp2_fin(x.v), x); }
    // d log2(x) = dx/(x ln2): one reciprocal of the argument for all tangents (dead code when every tangent is a structural zero)
    static __device__ __forceinline__ D log2_rule(FT l, const D &x) { return chain(l, FT(1.4426950408889634) * MS::rcp(x.v), x); }
    static __device__ __forceinline__ D log2(const D &x) { return log2_rule(MS::log2(x.v), x); }
    static __device__ __forceinline__ D log2_pn(const D &x) { return log2_rule(MS::log2_pn(x.v), x); }
    static __device__ __forceinline__ D rcp_rule(FT r, const D &x) { return chain(r, -(r * r), x); }
    static __device__ __forceinline__ D rcp(const D &x) { return rcp_rule(MS::rcp(x.v), x); }
    static __device__ __forceinline__ D rcp_nz(const D &x) { return rcp_rule(MS::rcp_nz(x.v), x); }
    static __device__ __forceinline__ D rcp_nz1(const D &x) { return rcp_rule(MS::rcp_nz1(x.v), x); }
    // d x^(−1/2) = −½ x^(−3/2) dx = −½ r³ dx
    static __device__ __forceinline__ D rsqrt_rule(FT r, const D &x) { return chain(r, FT(-0.5) * r * (r * r), x); }
    static __device__ __forceinline__ D rsqrt(const D &x) { return rsqrt_rule(MS::rsqrt(x.v), x); }
    static __device__ __forceinline__ D rsqrt_pos(const D &x) { return rsqrt_rule(MS::rsqrt_pos(x.v), x); }
    // d √x = dx/(2 √x): one reciprocal of the root for all tangents
    static __device__ __forceinline__ D sqrt_rule(FT s, const D &x) { return chain(s, FT(0.5) * MS::rcp(s), x); }
    static __device__ __forceinline__ D sqrt(const D &x) { return sqrt_rule(MS::sqrt(x.v), x); }
    static __device__ __forceinline__ D sqrt_pos(const D &x) { return sqrt_rule(MS::sqrt_pos(x.v), x); }
    template <typename A, typename B> static __device__ __forceinline__ D div(A a, B b) { return D(a) * rcp(D(b)); }
    // any mix of duals and scalars: the value is ONE fma of the values, like the plain instantiation's
    template <typename A, typename B, typename C> static __device__ __forceinline__ D fma(A a, B b, C c) {
        using namespace dual_detail;
        D r; r.v = MS::fma(val(a), val(b), val(c));
#pragma unroll
        CMX_DUAL_FOR r.d[k] = add(lin2((FT)val(b), (FT)tan(a, k), (FT)val(a), (FT)tan(b, k)), (FT)tan(c, k));
        return r;
    }
    // the value is the plain instantiation's max / min of the values (which returns the other operand for a NaN); the tangents are those of the operand
    // that value came from — the first one on a tie
    template <typename A, typename B> static __device__ __forceinline__ D max(A a, B b) {
        using namespace dual_detail;
        const FT x = val(a), y = val(b);
        const bool second = (y > x) || (x != x);
        D r; r.v = MS::max(x, y);
#pragma unroll
        CMX_DUAL_FOR r.d[k] = second ? (FT)tan(b, k) : (FT)tan(a, k);
        return r;
    }
    template <typename A, typename B> static __device__ __forceinline__ D min(A a, B b) {
        using namespace dual_detail;
        const FT x = val(a), y = val(b);
        const bool second = (y < x) || (x != x);
        D r; r.v = MS::min(x, y);
#pragma unroll
        CMX_DUAL_FOR r.d[k] = second ? (FT)tan(b, k) : (FT)tan(a, k);
        return r;
    }
};

// ---- the free functions of cmx_math.hpp for a dual (found by argument-dependent lookup from the point functions) ---------------------------------------
// keep(x): the VALUE is made opaque where the plain instantiation makes it opaque (cmx_math.hpp); the tangents need no such care
template <typename FT, int K> __device__ __forceinline__ Dual<FT, K> keep(Dual<FT, K> x) {
    x.v = keep(x.v);
    return x;
}
// max(0, x) of a loaded value: the plain max0 on the value; the tangents pass where x > 0 (the clamp is part of the differentiated function)
template <typename FT, int K> __device__ __forceinline__ Dual<FT, K> max0(const Dual<FT, K> &x) {
    Dual<FT, K> r; r.v = max0(x.v);
    const bool pass = x.v > FT(0);
#pragma unroll
    CMX_DUAL_FOR r.d[k] = pass ? x.d[k] : FT(0);
    return r;
}
// lo ≤ hi, both constants: the plain clamp_ordered on the value; the tangents pass strictly inside
template <typename FT, int K> __device__ __forceinline__ Dual<FT, K> clamp_ordered(const Dual<FT, K> &x, std::enable_if_t<true, FT> lo, std::enable_if_t<true, FT> hi) {
    Dual<FT, K> r; r.v = clamp_ordered(x.v, lo, hi);
    const bool pass = !(x.v < lo) && !(x.v > hi);
#pragma unroll
    CMX_DUAL_FOR r.d[k] = pass ? x.d[k] : FT(0);
    return r;
}
// lo ≤ hi with bounds that are duals themselves (the 1-moment cloud-ice excess is clamped to −q_icl, cmx_mp1m.hpp): the plain clamp_ordered on the values; a
// value clamped to a bound carries THAT BOUND's tangents (ForwardDiff's rule: the operand whose value is returned), x's on a tie and inside
template <typename FT, int K> __device__ __forceinline__ Dual<FT, K> clamp_ordered(const Dual<FT, K> &x, const Dual<FT, K> &lo, const Dual<FT, K> &hi) {
    Dual<FT, K> r; r.v = clamp_ordered(x.v, lo.v, hi.v);
    const bool below = x.v < lo.v, above = !below && x.v > hi.v;
#pragma unroll
    CMX_DUAL_FOR r.d[k] = below ? lo.d[k] : (above ? hi.d[k] : x.d[k]);
    return r;
}
template <typename FT, int K> __device__ __forceinline__ Dual<FT, K> clamp_ordered(const Dual<FT, K> &x, const Dual<FT, K> &lo, std::enable_if_t<true, FT> hi) {
    return clamp_ordered(x, lo, Dual<FT, K>(hi));
}
// log2 of a non-negative quantity that is ordinarily zero (cmx_math.hpp log2_floored): the value is formed exactly as there; Float64: the tangent is that of
// the operand the max returned — the literal zeros of the floor for an absent species; Float32: the logarithm's own rule (an absent species has −Inf with a
// non-finite tangent, which the floor of the slope parameter or the gate q > ϵ behind it discards)
template <typename FT, int K> __device__ __forceinline__ Dual<FT, K> log2_floored(const Dual<FT, K> &x) {
    using MD = Math<Dual<FT, K>>;
    if constexpr (MD::IS_F64) return MD::log2_pn(MD::max(x, FT(2.2250738585072014e-308)));
    else return MD::log2(x);
}
// a value that is constant wherever `gate` holds (cmx_math.hpp flat_where): no tangents there — the chain rule through the −Inf exponent that made it 0 would
// give 0·Inf
template <typename FT, int K> __device__ __forceinline__ Dual<FT, K> flat_where(bool gate, const Dual<FT, K> &x) {
    Dual<FT, K> r; r.v = x.v;
#pragma unroll
    CMX_DUAL_FOR r.d[k] = gate ? FT(0) : x.d[k];
    return r;
}
// Γ of the general Chen-2022 fall speed (cmx_math.hpp tgamma_general): its argument b_i(ρ) + 1 depends on the state through ρ only, which no entry
// differentiates — the value part, every tangent the literal zero
template <typename FT, int K> struct TGammaGeneral<Dual<FT, K>> {
    static __device__ __forceinline__ Dual<FT, K> eval(const Dual<FT, K> &z) { return Dual<FT, K>(tgamma_general<FT>(z.v)); }
};
// the phase boundary of the constants (cmx_math.hpp consts_after) waits for the VALUE
template <typename CT> struct holds_duals : std::false_type {};
template <template <typename> class CT, typename FT, int K> struct holds_duals<CT<Dual<FT, K>>> : std::true_type {};
template <typename C, typename FT, int K> __device__ __forceinline__ const C &consts_after(const C &c, const Dual<FT, K> &dep) { return consts_after(c, dep.v); }
#undef CMX_DUAL_FOR

// The constants a scheme's eval hands to its point function: front_consts (cmx_math.hpp) — unless the constants struct holds duals itself, as for the
// parameter derivatives (cmx_jacobian.hpp param_jvp_point).  Those stay the plain reference to the kernel argument in both float types: a class in the
// constant address space binds to no reference parameter of the operators above (tried: 30 errors in sb2006_point).  Tried as well, and measured (one MI355X,
// 1e7 points, ms per direction of the SB2006 parameter gradient at one direction per launch): the kernel-argument pointer cast to a plain one behind the empty
// asm of consts_after, per phase — the loads stay scalar and the Float64 kernel parks 190–196 instead of 292–340 SGPRs: Float64 0.58 → 0.50, Float32 0.18 → 0.22.
// Not kept: slower in Float32, and in Float64 two directions per launch gain more (0.35) without casting a plain pointer back into the constant address space.
template <typename FT, bool ALSO = false, typename CT> __device__ __forceinline__ decltype(auto) scheme_consts(const CT &c) {
    if constexpr (holds_duals<CT>::value) return (c);
    else return front_consts<FT, ALSO>(c);
}


}  // namespace cmx
