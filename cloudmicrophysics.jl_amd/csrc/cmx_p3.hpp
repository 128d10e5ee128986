// cmx_p3.hpp — shared device code of the P3 kernels (cmx_p3_kernels.hip: shape solver, fall speeds, melting, self-collection;
// cmx_p3_collisions.hip: liquid–ice collisions and the 2M+P3 fused entry): elementary-function traits, incomplete gamma
// function and its inverse, P3State construction, Chen-2022 ice fall-speed constants.  Reference lines are cited on each item.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cmx_launch.hpp"
#include "cmx_math.hpp"

// Floating-point contraction in the P3 code (round 5).  The library is built with -ffp-contract=off: a fused multiply-add is written where it is meant
// (Math<FT>::fma), so every kernel that shares a point function rounds alike and the host builds of the point functions (tests/native) round like the
// device.  The P3 quadrature integrands, incomplete-gamma recurrences and Brent arithmetic are the exception: long sums of products written term by term,
// shared with no host build, in kernels bound by VALU issue — contraction takes 10–17 % of the instructions out of their node loops (same-box A/B, ms per
// 1e6 / 1e7 states: 2M + P3 Float64 20.7 → 19.1, shape + fall speeds 26.8 → 24.5, self-collection 50.7 → 46.1; Float32 6.7 → 6.2, 8.0 → 7.1, 16.1 → 14.7).
// The pragma brackets exactly that code: this header's device functions and the P3 kernels of cmx_p3_kernels.hip / cmx_p3_collisions.hip.  The pointwise
// part of the 2M + P3 entry (mp2m_p3_point → sb2006_point) stays outside — it is bit-identical to the warm-rain entry, and tested so.
// The bracket acts in the DEVICE pass only: the host pass of the same sources holds the entry functions that fold the kernel constants
// (make_p3_consts, the collision entry), which the Python and oracle mirrors reproduce operation by operation — an FMA-capable host build must not contract
// them.  There both macros are empty, so the translation unit's own default stays in force.
#if defined(__HIP_DEVICE_COMPILE__)
#define CMX_P3_CONTRACT_BEGIN _Pragma("clang fp contract(fast)")
#define CMX_P3_CONTRACT_END _Pragma("clang fp contract(off)")
#else
#define CMX_P3_CONTRACT_BEGIN
#define CMX_P3_CONTRACT_END
#endif

namespace cmx {
CMX_P3_CONTRACT_BEGIN

// elementary functions for the solver (the residual is a log-sum-exp of incomplete-gamma moments): lean exp/log
// (cmx_lean_f64.hpp) in Float64, OCML for the rest and for Float32
template <typename FT> struct PM;
template <> struct PM<double> {
    // one-argument forms (the shape solver's dozen call sites around the incomplete-gamma loops; the quadrature loops use the
    // register-pinned lean forms below): the table-driven lean routines where the translation unit keeps their polynomial coefficients
    // as SGPR literals (cmx_lean_f64.hpp CMX_LEAN_COEFS_IN_LDS = 0: 253 VGPRs, 2 waves per SIMD like the OCML build, 10 % fewer
    // instructions — shape + fall speeds 41.7 → 38.5 ms per 1e7 columns, 2M + P3 27.9 → 26.7 ms per 1e6 states, same-box A/B round 2).
    // With the coefficients in LDS the inlined lean routines cost 286 VGPRs — 1 wave per SIMD, 24 → 30 ms (OCML served there): both
    // translation units that include this header are in the Makefile's LITCOEF list, and must stay there.
#if CMX_LEAN_COEFS_IN_LDS      // (defined in the device pass only)
#error "cmx_p3.hpp: the P3 translation units keep the lean Float64 coefficients as SGPR literals (csrc/Makefile LITCOEF); with them in LDS the shape solver needs 286 VGPRs"
#endif
    static __device__ __forceinline__ double log(double x) { return lean::log(x); }
    static __device__ __forceinline__ double exp(double x) { return lean::exp(x); }
    static __device__ __forceinline__ double lgamma(double x) { return lean::lgamma_pos(x); }   // every argument here is > 0 (μ + 1, μ + b + n + 1, 1 + b_j)
    static __device__ __forceinline__ double expm1(double x) { return ::expm1(x); }
    static __device__ __forceinline__ double log1p(double x) { return ::log1p(x); }
    static __device__ __forceinline__ double pow(double x, double y) { return ::pow(x, y); }
    static __device__ __forceinline__ double tanh(double x) { return ::tanh(x); }
    static __device__ __forceinline__ double atanh(double x) { return ::atanh(x); }
    static __device__ __forceinline__ double log2(double x) { return ::log2(x); }
    static __device__ __forceinline__ double abs(double x) { return __builtin_fabs(x); }
    // 1/d to ≈1 ulp: v_rcp_f64 (≈2⁻²⁴ relative) + two Newton steps — no div_scale / div_fmas / div_fixup sequence.
    // Only for finite, normal d (the incomplete-gamma loops: d = a + k, or a rescaled continued-fraction denominator).
    static __device__ __forceinline__ double rcp(double d) { return lean::rcp_finite(d); }
    // hot-loop variants with register-pinned constants (cmx_lean_f64.hpp): table-driven since round 2 (round 1: table-free polynomial
    // forms, 29 pinned values).  The kernels call Math<FT>::prepare() first (tables → LDS).
#ifndef CMX_P3_SCALAR_COEFS
#define CMX_P3_SCALAR_COEFS 0      // 1: the hot loops call the one-argument forms with SGPR-literal coefficients (needs CMX_LEAN_COEFS_IN_LDS=0)
#endif
#if CMX_P3_SCALAR_COEFS
    struct Coefs {};
    static __device__ __forceinline__ Coefs coefs() { return {}; }
    // the two-argument forms are the quadrature-integrand forms: their exponents are finite combinations of ln D, D and per-state
    // constants at interior nodes D > 0 — the finite-argument exponential (no clamp, no NaN select; NaN still propagates)
    static __device__ __forceinline__ double exp(double x, const Coefs &) { return lean::exp_fin(x); }
    static __device__ __forceinline__ double log(double x, const Coefs &) { return lean::log(x); }
    static __device__ __forceinline__ double log_pos(double x, const Coefs &) { return lean::log_pos(x); }   // positive normal finite x
#else
    using Coefs = lean::TabCoefs;
    static __device__ __forceinline__ Coefs coefs() { return lean::tab_coefs(); }
    static __device__ __forceinline__ double exp(double x, const Coefs &k) { return lean::exp_fin(x, k); }   // integrand form: see above
    static __device__ __forceinline__ double log(double x, const Coefs &k) { return lean::log(x, k); }
    static __device__ __forceinline__ double log_pos(double x, const Coefs &k) { return lean::log_pos(x, k); }
#endif
    // Constants pinned in registers for ONE phase of a kernel built with the scalar forms (round 5): the phase with register slack pays for them, the phase
    // at the kernel's register limit (the collision sweep) keeps the scalar forms.  Pinned are all eighteen constants of the table-driven exp / log
    // (lean::tab_coefs — volatile pins, so they are born where coefs_local() is called and not before).  Measured against pinning only the second
    // polynomial coefficient of each (no v_mov_b64 in front of the first Horner step) and against the scalar forms everywhere
    // (profiles/r05_ab_sessions.txt session 9): 20.7 ms against 21.0 and 21.2.
#if CMX_P3_SCALAR_COEFS
    // every constant of the table-driven exp / log in registers for the phase (18 pairs, the TabCoefs of the translation units that are not at a register limit)
    using LocalCoefs = lean::TabCoefs;
    static __device__ __forceinline__ LocalCoefs coefs_local(double) { return lean::tab_coefs(); }
    static __device__ __forceinline__ double exp(double x, const LocalCoefs &k) { return lean::exp_fin(x, k); }
    static __device__ __forceinline__ double log_pos(double x, const LocalCoefs &k) { return lean::log_pos(x, k); }
#else
    using LocalCoefs = Coefs;
    static __device__ __forceinline__ LocalCoefs coefs_local(double) { return coefs(); }
#endif
    static __device__ __forceinline__ void pin(double &x) { lean::pin(x); }
    static __device__ __forceinline__ double exp_fast(double x) { return exp(x); }       // Float64: the one-argument forms above
    static __device__ __forceinline__ double log_fast(double x) { return log(x); }
    static constexpr int kBrent = 10, kGammaIters = 30;      // P3_size_distribution.jl:311, Utilities.jl:104
    static constexpr int kRescale = 6;                        // continued-fraction rescale period (b ≤ 1e8 → 1e48 growth)
    static constexpr double eps() { return 2.220446049250313e-16; }
};
template <> struct PM<float> {
    static __device__ __forceinline__ float log(float x) { return ::logf(x); }
    static __device__ __forceinline__ float exp(float x) { return ::expf(x); }
    static __device__ __forceinline__ float lgamma(float x) { return ::lgammaf(x); }
    static __device__ __forceinline__ float expm1(float x) { return ::expm1f(x); }
    static __device__ __forceinline__ float log1p(float x) { return ::log1pf(x); }
    static __device__ __forceinline__ float pow(float x, float y) { return ::powf(x, y); }
    static __device__ __forceinline__ float tanh(float x) { return ::tanhf(x); }
    static __device__ __forceinline__ float atanh(float x) { return ::atanhf(x); }
    static __device__ __forceinline__ float log2(float x) { return ::log2f(x); }
    static __device__ __forceinline__ float abs(float x) { return __builtin_fabsf(x); }
    struct Coefs {};
    static __device__ __forceinline__ Coefs coefs() { return {}; }
    using LocalCoefs = Coefs;
    static __device__ __forceinline__ LocalCoefs coefs_local(float) { return {}; }
    static __device__ __forceinline__ void pin(float &) {}
    // the incomplete-gamma prefactor e^(a ln x − x − ln Γ(a)) — eight per residual evaluation of the shape solver — takes the hardware forms too
    // (OCML's expf / logf before)
    static __device__ __forceinline__ float exp_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
    static __device__ __forceinline__ float log_fast(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }
    // hot-loop forms (quadrature integrands): the hardware v_exp_f32 / v_log_f32 with one multiply — 2 instructions instead of OCML's 15
    // (expf) and 14 (logf), which spend the rest on the last ulp and on subnormals; the product x·log₂e is rounded once, so the
    // relative error is ≈ 6e-8·(1 + |x| log₂e) (1e-5 at |x| = 100) — an integrand weight, well inside the 1e-3 Float32 bound.  The shape
    // solver and the set-up code keep the one-argument OCML forms.
    static __device__ __forceinline__ float exp(float x, const Coefs &) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
    static __device__ __forceinline__ float log(float x, const Coefs &) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }
    static __device__ __forceinline__ float log_pos(float x, const Coefs &k) { return log(x, k); }      // Float32: the hardware form handles every class
    static __device__ __forceinline__ float rcp(float d) {
        const float r = __builtin_amdgcn_rcpf(d);
        return __builtin_fmaf(r, __builtin_fmaf(-d, r, 1.0f), r);
    }
    static constexpr int kBrent = 8, kGammaIters = 20;
    static constexpr int kRescale = 2;                        // Float32: (1e8)² < 3e38
    static constexpr float eps() { return 1.1920928955078125e-07f; }
};

#if CMX_HAVE_PACKED
// Two quadrature nodes per value (round 6): the node loops of the Float32 fall-speed / melting integrals evaluate PAIRS of nodes in packed arithmetic
// (cmx_math.hpp f32x2) — the transcendentals, compares and selects run per half, the ≈ 30 multiplies / adds / fmas of a node as v_pk_* instructions.
template <> struct PM<f32x2> {
    using Coefs = PM<float>::Coefs;
    static __device__ __forceinline__ f32x2 exp(f32x2 x, const Coefs &k) { return f32x2{PM<float>::exp(x.x, k), PM<float>::exp(x.y, k)}; }
    static __device__ __forceinline__ f32x2 log_pos(f32x2 x, const Coefs &k) { return f32x2{PM<float>::log_pos(x.x, k), PM<float>::log_pos(x.y, k)}; }
    static __device__ __forceinline__ f32x2 abs(f32x2 x) { return __builtin_elementwise_abs(x); }
};
#endif
// ---- Brent's method with a fixed number of function evaluations ----------------------------------------------------------------------------------
// RootSolvers.BrentsMethod under the reference's FixedIterations tolerance (src/P3_size_distribution.jl:250-251,311-319; src/P3_processes.jl:325-334).
// RootSolvers' source is not vendored: the algorithm is Brent's zeroin (Brent 1973, ch. 4; netlib zeroin.f, Numerical Recipes zbrent) with t = 0 — the
// restatement that satisfies the reference's own warm-start suite (test/p3_shape_solver_warmstart_tests.jl, tests/test_reference_suites*.py), which the
// Wikipedia pseudo-code variant of rounds 1–5 fails (oracle/cmx_oracle_p3_impl.h o_brent_fixed holds both).  Same operations in the same order as the
// oracle's.  Usage: start(); then per evaluation: if (!order()) stop; x = propose(); accept(f(x)); after the last evaluation order() once more: b is
// the better end.
template <typename FT> struct Zeroin {
    FT a, b, c, fa, fb, fc, d, e;      // b: current iterate, a: the previous one, c: the end with the other sign; d: the step, e: the one before
    __device__ __forceinline__ void start(FT lo, FT hi, FT f_lo, FT f_hi) {
        a = lo; b = hi; fa = f_lo; fb = f_hi; c = a; fc = fa; d = b - a; e = d;
    }
    __device__ __forceinline__ FT tol1() const { return FT(2) * PM<FT>::eps() * PM<FT>::abs(b); }
    // orders the ends; false once the bracket has collapsed to 2 eps |b| or f(b) = 0
    __device__ __forceinline__ bool order() {
        using P = PM<FT>;
        if ((fb > FT(0) && fc > FT(0)) || (fb < FT(0) && fc < FT(0))) { c = a; fc = fa; d = b - a; e = d; }
        if (P::abs(fc) < P::abs(fb)) { a = b; b = c; c = a; fa = fb; fb = fc; fc = fa; }
        return !(P::abs((c - b) / FT(2)) <= tol1() || fb == FT(0));
    }
    // the next abscissa: inverse quadratic interpolation / secant where it stays inside and shrinks fast enough, else bisection
    __device__ __forceinline__ FT propose() {
        using P = PM<FT>;
        const FT t1 = tol1(), xm = (c - b) / FT(2);
        if (P::abs(e) >= t1 && P::abs(fa) > P::abs(fb)) {
            const FT sq = fb / fa;
            FT pp, q;
            if (a == c) { pp = FT(2) * xm * sq; q = FT(1) - sq; }
            else {
                const FT qa = fa / fc, r = fb / fc;
                pp = sq * (FT(2) * xm * qa * (qa - r) - (b - a) * (r - FT(1)));
                q = (qa - FT(1)) * (r - FT(1)) * (sq - FT(1));
            }
            if (pp > FT(0)) q = -q;
            pp = P::abs(pp);
            if (FT(2) * pp < Math<FT>::min(FT(3) * xm * q - P::abs(t1 * q), P::abs(e * q))) { e = d; d = pp / q; }
            else { d = xm; e = d; }
        } else { d = xm; e = d; }
        a = b; fa = fb;
        b += P::abs(d) > t1 ? d : (xm > FT(0) ? t1 : -t1);
        return b;
    }
    __device__ __forceinline__ void accept(FT f_b) { fb = f_b; }
};

template <typename FT> struct P3Consts {
    uint32_t flags;
    int32_t brent_iters;   // fixed Brent iteration budget (P3_size_distribution.jl:311: 8 Float32 / 10 Float64)
    FT alpha_va, beta_va, slope_a, slope_b, slope_c, mu_max, mu_const, rho_i, rho_l_08;
    FT p_inv;            // 1/(3 − β_va)
    FT six_alpha_pi;     // 6 α_va / π
    FT a_sph_i, D_th;    // ρ_i π/6, (6 α_va/(π ρ_i))^(1/(3−β_va))
    FT pi_6;
};

template <typename FT, typename PR> static P3Consts<FT> make_p3_consts(const PR &p, uint32_t flags) {
    P3Consts<FT> c{};
    const double pi = 3.14159265358979323846;
    c.flags = flags;
    c.alpha_va = (FT)p.alpha_va; c.beta_va = (FT)p.beta_va;
    c.slope_a = (FT)p.slope_a; c.slope_b = (FT)p.slope_b; c.slope_c = (FT)p.slope_c; c.mu_max = (FT)p.mu_max; c.mu_const = (FT)p.mu_const;
    c.rho_i = (FT)p.rho_i; c.rho_l_08 = (FT)(0.8 * (double)p.rho_l);
    c.p_inv = (FT)(1.0 / (3.0 - (double)p.beta_va));
    c.six_alpha_pi = (FT)(6.0 * (double)p.alpha_va / pi);
    c.a_sph_i = (FT)((double)p.rho_i * pi / 6.0);
    c.D_th = (FT)std::pow(6.0 * (double)p.alpha_va / (pi * (double)p.rho_i), 1.0 / (3.0 - (double)p.beta_va));
    c.pi_6 = (FT)(pi / 6.0);
    return c;
}

// UT.gamma_inc — Utilities.jl:93-144: series for x < a+1, Lentz continued fraction otherwise, both with a FIXED
// number of terms (20 Float32 / 30 Float64).  The device evaluates the same truncations in cheaper arithmetic:
//   * series: Σ_k x^k / (a(a+1)…(a+k)) as a fraction carried from the last term inwards (no division per term, see below);
//   * continued fraction: the n-th convergent h_n = A_n/B_n of  1/(b₀+ a₁/(b₁+ a₂/(b₂+…)))  by the forward (Wallis)
//     recurrence A_n = b_n A_{n−1} + a_n A_{n−2} — the value modified Lentz produces with two divisions per term —
//     rescaled every kRescale terms; one reciprocal at the end.
// `gamma_series` / `gamma_cf` return the bracketed sums WITHOUT the prefactor x^a e^{−x}/Γ(a).
template <typename FT> __device__ __forceinline__ FT gamma_series_sum(FT a, FT x) {
    using P = PM<FT>;
    // Σ_{k=0}^{K} x^k/(a(a+1)…(a+k)) = T₁/a with T_k = 1 + x T_{k+1}/(a+k), T_{K+1} = 1, carried as a fraction p/q from the last term
    // inwards: p ← q(a+k) + x p, q ← q(a+k) — three instructions per term and NO reciprocal (the term-by-term form spends one per
    // term: 8 instructions + a quarter-rate v_rcp in Float64), rescaled every kSeriesRescale terms ((a+k) ≤ 60: 6e17 / 8e8 growth).
    constexpr int R = sizeof(FT) == 8 ? 10 : 5;
    static_assert(P::kGammaIters % R == 0, "rescale period must divide the term count");
    if constexpr (sizeof(FT) == 4) {
        // Float32: forwards, S_k = M_k/D_k with M_k = M_{k−1}(a+k) + x^k, D_k = D_{k−1}(a+k) — four instructions per term, but the
        // terms fall monotonically (x < a + 1), so the wave can stop once the remaining tail is ≤ eps·S_k for all of its lanes in this loop
        FT M = FT(1), D = a, X = FT(1);
#pragma unroll 1
        for (int k0 = 0; k0 < P::kGammaIters; k0 += R) {
#pragma unroll
            for (int j = 1; j <= R; ++j) {
                const FT ak = a + FT(k0 + j);
                X *= x;
                M = Math<FT>::fma(M, ak, X);
                D *= ak;
            }
            // exit once the NEGLECTED TAIL is below eps of the sum, not merely the last term: the terms fall like
            // ρ_k = x/(a+k+1), so the tail after term k is ≤ term·ρ/(1 − ρ) = (X/D)·x/(a+k+1 − x); close to x = a + 1 with large a the
            // ratio is near 1 and the last term alone under-estimates the tail many times over
            const FT a_next = a + FT(k0 + R + 1);
            const bool done = X * x <= P::eps() * M * (a_next - x);
            const FT r = P::rcp(D);
            M *= r; X *= r; D = FT(1);
            if (__all(done)) break;
        }
        return M;       // D == 1
    }
    // Float64
    FT p = FT(1), q = FT(1);
    FT ak = a + FT(P::kGammaIters);      // a + k carried downwards: one subtraction per term instead of an integer conversion and an addition
#pragma unroll 1
    for (int k0 = P::kGammaIters; k0 > 0; k0 -= R) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const FT qa = q * ak;
            ak -= FT(1);
            p = Math<FT>::fma(x, p, qa);
            q = qa;
        }
        p *= P::rcp(q);
        q = FT(1);
    }
    return p * P::rcp(a);
}
template <typename FT> __device__ __forceinline__ FT gamma_cf_value(FT a, FT x) {
    using P = PM<FT>;
    static_assert(P::kGammaIters % P::kRescale == 0, "rescale period must divide the term count");
    // h₀ = 1/b₀:  A₀ = 1, B₀ = b₀;  A₋₁ = 0, B₋₁ = 1
    const FT b0 = x + FT(1) - a;
    if constexpr (sizeof(FT) == 8) {
        // Float64 (round 5): the SAME convergent h_N, evaluated from the tail inwards.  t_N = b_N, t_{k−1} = b_{k−1} + a_k/t_k, h_N = 1/t_0, with t carried as a
        // fraction p/q:  p ← b_{k−1} p + a_k q,  q ← p  — one multiply and one fused multiply-add per term where the forward (Wallis) recurrence above runs
        // two of each (A and B), and no convergent is formed on the way: Float64 never took the early exit (it reaches eps only near the full count).  The
        // coefficients by differences (a_{k−1} − a_k = 2k − 1 − a, b_{k−1} − b_k = −2: three additions per term); rescaled every kRescale terms by 1/p.
        // 8.5 → 6 instructions per term against the forward recurrence with difference coefficients.  The accumulated rounding of a_k is ≤ k ulp of a
        // number of size k² (1e-14 relative at the 30th term, against the 1e-6 of the parity bound and the 1e-11 the shape solve reaches).
        constexpr int N = P::kGammaIters;
        FT bk = b0 + FT(2 * N);                      // b_N
        FT ak = -FT(N) * (FT(N) - a);                // a_N
        FT dk = FT(2 * N - 1) - a;                   // a_{N−1} − a_N
        FT p = bk, q = FT(1);
#pragma unroll 1
        for (int k0 = N; k0 > 0; k0 -= P::kRescale) {
#pragma unroll
            for (int j = 0; j < P::kRescale; ++j) {
                bk -= FT(2);
                const FT pn = Math<FT>::fma(bk, p, ak * q);
                q = p; p = pn;
                ak += dk; dk -= FT(2);
            }
            q *= P::rcp(p); p = FT(1);
        }
        return q;
    }
    // Float32: the forward recurrence with closed-form coefficients
    FT Am = FT(0), Bm = FT(1), A = FT(1), B = b0;
    FT A_prev = FT(0);
#pragma unroll 1
    for (int k0 = 0; k0 < P::kGammaIters; k0 += P::kRescale) {
#pragma unroll
        for (int j = 1; j <= P::kRescale; ++j) {
            const FT kk = FT(k0 + j);
            const FT ak = -kk * (kk - a), bk = b0 + FT(2) * kk;
            const FT An = bk * A + ak * Am, Bn = bk * B + ak * Bm;
            Am = A; Bm = B; A = An; B = Bn;
        }
        const FT r = P::rcp(B);
        A *= r; Am *= r; Bm *= r; B = FT(1);
        // the reference's 20 / 30 terms are an upper bound: stop once the convergent no longer moves for ANY lane of the wave that is in
        // this loop (after a rescale A IS the convergent; a NaN compares unequal forever and runs the full count)
        // Float32 only (same-box A/B, shape + fall speeds per 1e7 columns: 13.1 → 11.75 ms; Float64 reaches eps only near the full count:
        // 29.5 → 29.6 ms with the test)
        if constexpr (sizeof(FT) == 4) {
            if (__all(P::abs(A - A_prev) <= P::eps() * P::abs(A))) break;
            A_prev = A;
        }
    }
    return A;
}
template <typename FT> __device__ FT gamma_inc_dev(FT a, FT x, FT lgam_a, bool want_P) {
    using P = PM<FT>;
    if (x <= FT(0)) return want_P ? FT(0) : FT(1);
    if (isinf(x)) return want_P ? FT(1) : FT(0);
    const FT factor = P::exp_fast(a * P::log_fast(x) - x - lgam_a);
    const bool series = x < a + FT(1);
    const FT body = series ? gamma_series_sum<FT>(a, x) : gamma_cf_value<FT>(a, x);
    const FT pq = Math<FT>::min(Math<FT>::max(factor * body, FT(0)), FT(1));   // P on the series branch, Q on the other
    return (series == want_P) ? pq : FT(1) - pq;
}

// A kernel-argument constant used as one side of a per-lane select.  Without this the optimiser rewrites `c ? k.a : k.b` (two uniform scalar
// loads) into a load of the SELECTED ADDRESS — a per-lane vector load from the kernel-argument segment inside the quadrature loops (round 3:
// two such loads per inner node of the self-collection integral, with three waves per SIMD to hide them).  The empty asm makes the loaded
// value opaque in an SGPR, so the select stays a select of registers.  Float32 only (self-collection 19.8 → 19.5 ms per 1e6 states, same-box
// A/B): in the Float64 kernels the SGPR file is over-subscribed and the pinned constants are re-loaded with scalar loads + s_waitcnt inside the
// loop (2M + P3 22.2 → 30.2 ms, self-collection 62.4 → 76.4 — measured, reverted); there the vector loads, whose latency the other waves hide,
// are the better code.
template <typename FT> __device__ __forceinline__ FT kpin(FT x) {
    if constexpr (sizeof(FT) == 4) asm volatile("" : "+s"(x));
    return x;
}

template <typename FT> struct P3Point {
    FT rho_q, rho_n, F_rim, rho_rim, rho_g;
    FT bnd[5];          // 0, D_th, D_gr, D_cr, ∞          segment_boundaries :280-291
    FT log_a[4], b[4];  // ice_mass_coeffs at each segment's midpoint :346-356
};

template <typename FT> __device__ __forceinline__ FT p3_mu(const P3Consts<FT> &c, FT loglam) {   // get_μ :171-173
    using P = PM<FT>;
    if (c.flags & CMX_P3_SLOPE_CONSTANT) return c.mu_const;
    return Math<FT>::min(Math<FT>::max(c.slope_a * P::exp(c.slope_b * loglam) - c.slope_c, FT(0)), c.mu_max);
}

// logmass_gamma_moment(state, μ, logλ; n) — :193-200 with loggamma_inc_moment :97-109 and unrolled_logsumexp
template <typename FT> __device__ FT p3_logmass_moment(const P3Consts<FT> &c, const P3Point<FT> &s, FT mu, FT loglam, FT n) {
    using P = PM<FT>;
    const FT lam = P::exp(loglam);
    // lgamma for the two distinct z: b = 3 (spherical regimes) and b = β_va (power-law regimes)
    const FT z_sph = FT(3) + n + mu + FT(1), z_pow = c.beta_va + n + mu + FT(1);
    const FT lg_sph = P::lgamma(z_sph), lg_pow = P::lgamma(z_pow);
    FT m[4];
    FT xmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const FT D1 = s.bnd[i], D2 = s.bnd[i + 1];
        FT val = -INFINITY;
        if (D1 < D2) {
            const bool sph = s.b[i] == FT(3);
            const FT z = sph ? z_sph : z_pow, lg = sph ? lg_sph : lg_pow;
            const FT x1 = D1 * lam, x2 = D2 * lam;
            const bool use_P = x2 < z + FT(1);
            const FT g1 = gamma_inc_dev<FT>(z, x1, lg, use_P), g2 = gamma_inc_dev<FT>(z, x2, lg, use_P);
            FT dq = use_P ? g2 - g1 : g1 - g2;
            dq = Math<FT>::max(dq, P::eps());
            val = -z * loglam + lg + P::log(dq) + s.log_a[i];
        }
        m[i] = val;
        xmax = (val > xmax || isnan(val)) ? val : xmax;
    }
    if (!isfinite(xmax)) return xmax;
    FT sum = FT(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) sum += P::exp(m[i] - xmax);
    return xmax + P::log(sum);
}

template <typename FT> __device__ __forceinline__ FT p3_logLdivN(const P3Consts<FT> &c, const P3Point<FT> &s, FT loglam) {   // :211-216
    const FT mu = p3_mu<FT>(c, loglam);
    return p3_logmass_moment<FT>(c, s, mu, loglam, FT(0)) - (-(mu + FT(1)) * loglam + PM<FT>::lgamma(mu + FT(1)));
}

template <typename FT> __device__ __forceinline__ FT exprel1(FT x) { return PM<FT>::expm1(x) / x; }
template <typename FT> __device__ __forceinline__ FT exprel2(FT x) {   // P3_particle_properties.jl:161-166
    using P = PM<FT>;
    if (P::abs(x) < FT(0.2)) {
        FT r = FT(1.0 / 362880);
        r = r * x + FT(1.0 / 40320); r = r * x + FT(1.0 / 5040); r = r * x + FT(1.0 / 720); r = r * x + FT(1.0 / 120);
        r = r * x + FT(1.0 / 24); r = r * x + FT(1.0 / 6); r = r * x + FT(0.5);
        return r;
    }
    return (P::expm1(x) - x) / (x * x);
}
template <typename FT> __device__ __forceinline__ FT regularised_ratio(FT num, FT den) {   // Utilities.jl:445-488
    using P = PM<FT>;
    const FT half = P::eps();
    FT w;
    if (den < FT(0)) w = FT(0);
    else if (den > Math<FT>::min(FT(1), FT(42) * half)) w = FT(1);
    else if (FT(4) * den < P::eps()) w = FT(0);
    else w = (FT(1) + P::tanh(FT(2) * P::atanh(FT(1) - FT(2) * P::pow(FT(1) - den, FT(-1) / P::log2(FT(1) - half))))) / FT(2);
    return den < P::eps() * P::eps() ? FT(0) : w * num / den;
}

template <typename FT> struct P3IO { const FT *rho_q, *rho_n, *x3, *x4, *guess; FT *F_rim, *rho_rim, *loglam, *D_m, *logN0; };

// ice_mass_coeffs at the midpoint of segment k (regime_value :320-332, :346-356): m(D) = a D^b.  From the thresholds and ρ_g of the point —
// a kernel that needs the coefficients of one segment late (the melting sweep of the 2M + P3 entry) re-derives them with this instead of
// keeping the eight values of P3Point::log_a / b alive across its other sweeps
template <typename FT> struct P3Point;
template <typename FT>
__device__ __forceinline__ void p3_mass_law_at(const P3Consts<FT> &c, const P3Point<FT> &s, FT D, FT &a, FT &b);
template <typename FT>
__device__ __forceinline__ void p3_segment_mass_law(const P3Consts<FT> &c, const P3Point<FT> &s, int k, FT &a, FT &b) {
    p3_mass_law_at<FT>(c, s, (s.bnd[k] + s.bnd[k + 1]) / FT(2), a, b);
}
template <typename FT>
__device__ __forceinline__ void p3_mass_law_at(const P3Consts<FT> &c, const P3Point<FT> &s, FT D, FT &a, FT &b) {
    using P = PM<FT>;
    const bool unrimed = s.F_rim == FT(0);
    if (D < c.D_th) { a = c.a_sph_i; b = FT(3); }
    else if (unrimed) { a = c.alpha_va; b = c.beta_va; }
    else if (D < s.bnd[2]) { a = c.alpha_va; b = c.beta_va; }
    else if (D < s.bnd[3]) { a = s.rho_g * c.pi_6; b = FT(3); }
    else { a = c.alpha_va / Math<FT>::max(FT(1) - s.F_rim, P::eps()); b = c.beta_va; }
}

// state_from_prognostic :101-106 (or P3State from (F_rim, ρ_rim)) → P3State :43-56: ρ_d (exact solution :191-199), ρ_g,
// thresholds, and the per-segment mass-law coefficients (regime_value at the segment midpoint :320-332)
// (F_rim, ρ_rim) of state_from_prognostic :101-106 alone — all the pointwise part of the 2M + P3 entry needs of the state
template <typename FT>
__device__ __forceinline__ void p3_rime_state(const P3Consts<FT> &c, FT rho_q, FT x3, FT x4, FT &F_rim, FT &rho_rim) {
    using P = PM<FT>;
    if (c.flags & CMX_P3_INPUT_IS_STATE) {
        F_rim = x3; rho_rim = x4;
    } else {
        F_rim = Math<FT>::min(regularised_ratio<FT>(Math<FT>::min(x3, rho_q), rho_q), FT(1) - P::eps());
        rho_rim = Math<FT>::min(regularised_ratio<FT>(x3, x4), c.rho_l_08);
    }
}
template <typename FT>
__device__ __forceinline__ void p3_make_point(const P3Consts<FT> &c, FT rho_q, FT rho_n, FT x3, FT x4, P3Point<FT> &s) {
    using P = PM<FT>;
    s.rho_q = rho_q; s.rho_n = rho_n;
    p3_rime_state<FT>(c, rho_q, x3, x4, s.F_rim, s.rho_rim);
    {
        const FT p = c.p_inv, logFu = P::log1p(-s.F_rim);
        const FT phi1 = exprel1<FT>(logFu), phi1mp = exprel1<FT>((FT(1) - p) * logFu);
        const FT H = -p * exprel2<FT>(-p * logFu) - (FT(1) - p) * exprel2<FT>((FT(1) - p) * logFu);
        const FT rho_d = -(s.rho_rim * phi1 * phi1mp) / (H - phi1mp * phi1);
        s.rho_g = s.F_rim * s.rho_rim + (FT(1) - s.F_rim) * rho_d;
    }
    const bool unrimed = s.F_rim == FT(0);
    const FT D_gr = unrimed ? FT(INFINITY) : P::pow(c.six_alpha_pi / s.rho_g, c.p_inv);
    const FT D_cr = unrimed ? FT(INFINITY) : P::pow(c.six_alpha_pi / (s.rho_g * (FT(1) - s.F_rim)), c.p_inv);
    s.bnd[0] = FT(0); s.bnd[1] = c.D_th; s.bnd[2] = D_gr; s.bnd[3] = D_cr; s.bnd[4] = FT(INFINITY);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        FT a, b;
        p3_segment_mass_law<FT>(c, s, k, a, b);
        s.log_a[k] = P::log(a); s.b[k] = b;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Number- and mass-weighted fall speeds — src/P3_terminal_velocity.jl:72-91,118-137.
//
// Per quadrature node the reference evaluates n(D)·v(D)[·m(D)] with ≈12 pow/exp/log/cbrt; here every factor is a
// power law or an exponential of D inside one mass-regime segment, so the whole integrand is assembled in the log
// domain from ONE log(D):  n·v = Σ_k A_k exp(base + e_k + b_k logD − c_k D),  base = logN₀ + μ logD − λD, where
//   * (A_k, e_k, b_k, c_k) are the Chen-2022 small- or large-ice terms (selected per node by D ≤ cutoff) with the
//     parameter-only table reductions at ρᵢ = 916.7 folded on the host and the ρₐ-dependent prefactors once per point;
//     the two terms have opposite signs and cancel to ≈1/200 of their size for small D, so the sum is formed as
//     e^{base+E₁}·(A₁ + A₂ e^{E₂−E₁}) — the large shared factor stays OUTSIDE the difference, as D^b does in the reference;
//   * the aspect factor cbrt(ϕᵢ) is exactly 1 on the two spherical segments (small ice, graupel), a pure power law
//     of D on the unrimed / dense-rimed segment (folded into e_k, b_k: no extra transcendental), and needs the mixed
//     area F·πD²/4 + (1−F)·γD^σ only on the partially-rimed segment (one exp + one log more);
//   * m(D) = exp(log a_seg + b_seg logD) with the per-segment mass law of the shape solver.
// → 3–4 transcendentals per node (log D, exp of the shared factor, exp of the term ratio[, D^β]) instead of ≈12; nodes/weights are wave-uniform scalar loads from the kernel arguments.
template <typename FT> struct P3VelConsts {
    // small ice (table B3 reduced at ρᵢ): aᵢ = (Es, Fs)·ρₐ^As·1000^b, b = Bs + ρₐ Cs, c = (0, 1000 Gs)
    FT s_A, s_B, s_C, s_E, s_F, s_c2;
    // large ice (table B5 reduced): a = (Bl ρₐ^Al 1000^Cl, El ρₐ^Al e^{Hl ρₐ} 1000^Fl), b = (Cl, Fl), c = (0, 1000 Gl)
    FT l_A, l_a1, l_b1, l_a2, l_H, l_b2, l_c2;
    FT cutoff, ln1000;
    FT g0, g1;          // unrimed / dense-rimed aspect factor: cbrt ϕ = exp(g0 + g1 logD)
    FT h0_num;          // partially rimed: cbrt ϕ = exp((h0_num − log Fu)/3 + β/3 logD − ½ log area)
    FT pi_4, gamma_area, sigma_area;
    FT sqrt_gamma_pi, half_sigma;                        // collision radius of the non-spherical regime: √(γ/π)·D^(σ/2)
    FT p_lo, p_hi;      // FT(p), FT(1 − p)
    // ice_melt (P3_processes.jl:64-94): F_v = vent_a + vent_bc √(D v), vent_bc = b_v ∛(ν/D_v)/√ν; L_f(T) = LH_f0 + dcp_f (T − T_0)
    FT vent_a, vent_bc, K4, LH_f0, dcp_f, T_0, T_freeze;
};

template <typename FT, typename PR, typename VR>
static P3VelConsts<FT> make_p3_vel_consts(const PR &pr, const VR &vel, double p) {
    P3VelConsts<FT> v{};
    const double pi = 3.14159265358979323846, rho_i = 916.7;   // src/P3_terminal_velocity.jl:41
    const double l = std::log(rho_i), sq = std::sqrt(rho_i);
    const auto &s = vel.small_ice;
    const auto &g = vel.large_ice;
    v.s_A = (FT)((double)s.A[1] * l * l - (double)s.A[2] * l + (double)s.A[0]);
    v.s_B = (FT)(1.0 / ((double)s.B[0] + (double)s.B[1] * l + (double)s.B[2] / sq));
    v.s_C = (FT)((double)s.C[0] + (double)s.C[1] * std::exp((double)s.C[2] * rho_i) + (double)s.C[3] * sq);
    v.s_E = (FT)((double)s.E[0] - (double)s.E[1] * l * l + (double)s.E[2] * sq);
    v.s_F = (FT)(-std::exp((double)s.F[0] - (double)s.F[1] * l * l + (double)s.F[2] * l));
    v.s_c2 = (FT)(1000.0 / ((double)s.G[0] + (double)s.G[1] / l - (double)s.G[2] * l / rho_i));
    const double Al = (double)g.A[0] + (double)g.A[1] * l + (double)g.A[2] / (rho_i * sq);
    const double Bl = std::exp((double)g.B[0] + (double)g.B[1] * l * l + (double)g.B[2] * l);
    const double Cl = std::exp((double)g.C[0] + (double)g.C[1] / l + (double)g.C[2] / rho_i);
    const double El = (double)g.E[0] + (double)g.E[1] * l * sq + (double)g.E[2] * sq;
    const double Fl = (double)g.F[0] + (double)g.F[1] * l - std::exp(std::log(-(double)g.F[2]) - rho_i);
    const double Gl = 1.0 / ((double)g.G[0] + (double)g.G[1] * l * sq + (double)g.G[2] / sq);
    const double Hl = (double)g.H[0] + (double)g.H[1] * rho_i * rho_i * sq + std::exp(std::log(-(double)g.H[2]) - rho_i);
    v.l_A = (FT)Al; v.l_a1 = (FT)(Bl * std::pow(1000.0, Cl)); v.l_b1 = (FT)Cl;
    v.l_a2 = (FT)(El * std::pow(1000.0, Fl)); v.l_H = (FT)Hl; v.l_b2 = (FT)Fl; v.l_c2 = (FT)(1000.0 * Gl);
    v.cutoff = (FT)s.cutoff; v.ln1000 = (FT)std::log(1000.0);
    const double al = (double)pr.alpha_va, be = (double)pr.beta_va, ga = (double)pr.gamma, si = (double)pr.sigma, ri = (double)pr.rho_i;
    v.g0 = (FT)(std::log(3.0 * std::sqrt(pi) * al / (4.0 * ri * ga * std::sqrt(ga))) / 3.0);
    v.g1 = (FT)((be - 1.5 * si) / 3.0);
    v.h0_num = (FT)std::log(3.0 * std::sqrt(pi) * al / (4.0 * ri));
    v.pi_4 = (FT)(pi / 4.0); v.gamma_area = (FT)ga; v.sigma_area = (FT)si;
    v.sqrt_gamma_pi = (FT)std::sqrt(ga / pi); v.half_sigma = (FT)(0.5 * si);
    v.p_lo = (FT)p; v.p_hi = (FT)(1.0 - p);
    return v;
}
// … of the collision integrals: their quantile levels are FT numbers, p = FT(0.00001) (P3_processes.jl:546)
template <typename FT, typename PR, typename VR>
static P3VelConsts<FT> make_p3_collision_vel_consts(const PR &pr, const VR &vel) {
    P3VelConsts<FT> v = make_p3_vel_consts<FT>(pr, vel, 1e-5);
    v.p_lo = FT(0.00001); v.p_hi = FT(1) - v.p_lo;
    return v;
}

// Host constants that more than one constants struct holds under the same member names, filled by one function each (K: the struct).
// ice_melt (P3_processes.jl:64-94): ventilation F_v = vent_a + vent_bc √(D v), 4 K_therm, L_f(T) = LH_f0 + dcp_f (T − T_0)
template <typename K, typename VT, typename AP, typename TH> inline void fill_melt_consts(K &k, const VT &vent, const AP &aps, const TH &tps) {
    using FT = decltype(k.vent_a);
    k.vent_a = (FT)vent.a;
    k.vent_bc = (FT)((double)vent.b * std::cbrt((double)aps.nu_air / (double)aps.D_vapor) / std::sqrt((double)aps.nu_air));
    k.K4 = (FT)(4.0 * (double)aps.K_therm);
    k.LH_f0 = (FT)((double)tps.LH_s0 - (double)tps.LH_v0); k.dcp_f = (FT)((double)tps.cp_l - (double)tps.cp_i);
    k.T_0 = (FT)tps.T_0;
}
// saturation vapour pressure over ice: p_sat = press_tr (T/T_tr)^ps_pow exp(ps_b (1/T_tr − 1/T))
template <typename K, typename TH> inline void fill_ice_saturation_consts(K &k, const TH &tps) {
    using FT = decltype(k.ps_pow);
    const double dcp_i = (double)tps.cp_v - (double)tps.cp_i, Rv = tps.R_v;
    k.ps_pow = (FT)(dcp_i / Rv); k.ps_b = (FT)(((double)tps.LH_s0 - dcp_i * (double)tps.T_0) / Rv); k.inv_T_tr = (FT)(1.0 / (double)tps.T_triple);
    k.press_tr = tps.press_triple; k.R_v = tps.R_v;
}

// the flags of the entries that take a P3 state
constexpr uint32_t kP3StateFlags = CMX_P3_INPUT_IS_STATE | CMX_P3_SLOPE_CONSTANT | CMX_P3_NO_ASPECT_RATIO;

// The common prologue of the P3 entries, in their order of checks: parameter structs and flag mask, the count rule (cmx_launch.hpp),
// quadrature order and — where the entry takes one (p non-null) — the quantile level, then n == 0.  proceed = false: the entry returns status.
struct P3Checked { int32_t status; bool proceed; };
template <typename FT, typename QUAD>
inline P3Checked p3_entry_checks(bool have_params, const QUAD *quad, uint32_t flags, uint32_t allowed, int64_t n, const FT *p) {
    if (!have_params || !quad || (flags & ~allowed)) return {CMX_ERR_BAD_ARG, false};
    if (const int32_t st = count_limit_status(n)) return {st, false};
    if (quad->n < 1 || quad->n > CMX_QUAD_MAX || (p && !(*p > FT(0) && *p < FT(0.5)))) return {CMX_ERR_BAD_ARG, false};
    return {CMX_OK, n != 0};
}

// UT._gamma_inc_inv — Utilities.jl:205-252 (Halley on P − p or Q − q, ≤ 15 iterations)
template <typename FT> __device__ FT gamma_inc_inv_dev(FT a, FT p, FT q) {
    using P = PM<FT>;
    if (p <= FT(0)) return FT(0);
    if (q <= FT(0)) return FT(INFINITY);
    const FT lg = P::lgamma(a);
    FT x = p < FT(0.5) ? P::exp((P::log(p) + lg + P::log(a)) / a) : a - P::log(q);   // (p Γ(a+1))^{1/a}
    const bool use_q = p > FT(0.5);
    for (int it = 0; it < 15; ++it) {
        const FT g = gamma_inc_dev<FT>(a, x, lg, !use_q);
        const FT f = use_q ? g - q : g - p;
        FT fprime = P::exp((a - FT(1)) * P::log(x) - x - lg);
        if (use_q) fprime = -fprime;
        if (fprime == FT(0)) break;
        const FT r = (a - FT(1) - x) / x;
        FT step = f / (fprime * (FT(1) - FT(0.5) * f * r / fprime));
        if (x - step <= FT(0)) step = FT(0.5) * x;
        x = x - step;
        if (P::abs(step) < P::eps() * x) break;
    }
    return x;
}

CMX_P3_CONTRACT_END
}  // namespace cmx
