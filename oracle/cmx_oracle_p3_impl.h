/*
 * cmx_oracle_p3_impl.h — oracle (TEST INFRASTRUCTURE) for the P3 ice scheme: state construction, regime
 * thresholds, the size-distribution shape solver and the mass-weighted mean diameter.
 * Included from cmx_oracle_impl.h (once per float type).  Restates, operation by operation:
 *   src/Utilities.jl        gamma_inc :93-144, unrolled_logsumexp :399-412, sgs_weight_function /
 *                           _regularised_ratio / rime_mass_fraction / rime_density :445-509
 *   src/P3_particle_properties.jl  P3State :43-56, state_from_prognostic :101-106, exprel :159-199,
 *                           get_ρ_d :191-199(+doc), get_ρ_g, thresholds :222-272, regime_value :320-332,
 *                           ice_mass_coeffs :346-356
 *   src/P3_size_distribution.jl    loggamma_inc_moment :97-109, loggamma_moment :151-157, get_μ :171-173,
 *                           logmass_gamma_moment :193-200, logLdivN :211-216, get_logN₀ :233-237,
 *                           get_distribution_logλ :284-320
 *   src/P3_integral_properties.jl  D_m :56-61
 * of the reference.  SpecialFunctions.loggamma → libm lgamma; LogExpFunctions.xexpy(x, y) = x·eʸ.
 * RootSolvers.jl (compat "0.3, 0.4, 1"; un-vendored, source ABSENT) BrentsMethod: the reference runs it for a FIXED number of
 * iterations (8 Float32 / 10 Float64, P3_size_distribution.jl:311).  Its iterates cannot be restated from source; what pins the
 * restatement is the reference's own warm-start suite (test/p3_shape_solver_warmstart_tests.jl:22-91, tests/golden/
 * reference_suites.json): the cold start and nine narrowed brackets of 72 states must agree to 1e-4 (Float64, 10 iterations) /
 * 1e-3 (Float32, 8).  o_brent_fixed below holds two candidates:
 *   variant 0 (default since round 6)  Brent's zeroin (Brent 1973, Algorithms for Minimization without Derivatives, ch. 4; the
 *              algorithm of netlib zeroin.f / Numerical Recipes zbrent) — passes that suite (worst 5e-7 at 10, 7e-4 at 8 iterations);
 *   variant 1 (rounds 1-5)             the pseudo-code of the Wikipedia article "Brent's method" (c := b every iteration: after a
 *              step that replaces `a` every proposal is refused until `b` moves) — FAILS it (1e-3 at 10, 3e-3 at 8 iterations),
 *              kept for the exposure measurement of tests/test_reference_suites.py; tests/test_p3_shape_roots.py selects it and asserts that failure.
 */
/* Quadrature rules beyond the ABI's struct (cmx_quadrature carries ≤ CMX_QUAD_MAX = 128 nodes; the reference's quadrature-order sweep compares
 * against order 200, test/bulk_tendencies_quadrature_tests.jl:232): a rule set here replaces the `quad` argument of every P3 integral of this
 * float type until it is cleared with n = 0.  Test infrastructure like the rest of the oracle; not thread-safe against concurrent setters. */
#define CMXO_QUAD_OVERRIDE_MAX 1024
static int FN(g_quad_n) = 0;
static FT FN(g_quad_node)[CMXO_QUAD_OVERRIDE_MAX], FN(g_quad_weight)[CMXO_QUAD_OVERRIDE_MAX];
int32_t FN(cmxo_set_quadrature_override)(int32_t n, const FT *node, const FT *weight) {
    if (n < 0 || n > CMXO_QUAD_OVERRIDE_MAX) return -1;
    for (int i = 0; i < n; ++i) { FN(g_quad_node)[i] = node[i]; FN(g_quad_weight)[i] = weight[i]; }
    FN(g_quad_n) = n;
    return 0;
}
#ifndef Q_N
#define Q_N(q) (FN(g_quad_n) > 0 ? FN(g_quad_n) : (q)->n)
#define Q_NODE(q, i) (FN(g_quad_n) > 0 ? FN(g_quad_node)[i] : (q)->node[i])
#define Q_WEIGHT(q, i) (FN(g_quad_n) > 0 ? FN(g_quad_weight)[i] : (q)->weight[i])
#endif
static int FN(g_brent_variant) = 0;
void FN(cmxo_set_brent_variant)(int32_t v) { FN(g_brent_variant) = v; }
typedef FT (*TY(cmxo_fn1))(FT x, const void *ctx);
/* the root of f on the bracket (a, b) with f(a) f(b) ≤ 0 after exactly `maxiters` further function evaluations (fewer once converged) */
static inline FT FN(o_brent_fixed)(TY(cmxo_fn1) f, const void *ctx, FT a, FT b, FT fa, FT fb, int maxiters) {
    if (FN(g_brent_variant) == 1) {
        if (M_ABS(fa) < M_ABS(fb)) { FT t = a; a = b; b = t; t = fa; fa = fb; fb = t; }
        FT c = a, fc = fa, d = 0;
        int mflag = 1;
        for (int it = 0; it < maxiters; ++it) {
            if (fb == 0 || a == b) break;
            FT sx;
            if (fa != fc && fb != fc)
                sx = a * fb * fc / ((fa - fb) * (fa - fc)) + b * fa * fc / ((fb - fa) * (fb - fc)) + c * fa * fb / ((fc - fa) * (fc - fb));
            else
                sx = b - fb * (b - a) / (fb - fa);
            FT lo3 = (3 * a + b) / 4;
            int out_of_range = !((sx > FN(o_min)(lo3, b)) && (sx < FN(o_max)(lo3, b)));
            if (out_of_range || (mflag && M_ABS(sx - b) >= M_ABS(b - c) / 2) || (!mflag && M_ABS(sx - b) >= M_ABS(c - d) / 2)) {
                sx = (a + b) / 2;
                mflag = 1;
            } else {
                mflag = 0;
            }
            FT fs = f(sx, ctx);
            d = c; c = b; fc = fb;
            if (fa * fs < 0) { b = sx; fb = fs; } else { a = sx; fa = fs; }
            if (M_ABS(fa) < M_ABS(fb)) { FT t = a; a = b; b = t; t = fa; fa = fb; fb = t; }
        }
        return b;
    }
    /* Brent's zeroin with t = 0: b the current iterate, a the previous one, c the end with the other sign; d the step, e the one before */
    FT c = a, fc = fa, d = b - a, e = d;
    for (int it = 0;; ++it) {
        if ((fb > 0 && fc > 0) || (fb < 0 && fc < 0)) { c = a; fc = fa; d = b - a; e = d; }
        if (M_ABS(fc) < M_ABS(fb)) { a = b; b = c; c = a; fa = fb; fb = fc; fc = fa; }
        FT tol1 = 2 * M_EPS * M_ABS(b), xm = (c - b) / 2;
        if (it >= maxiters || M_ABS(xm) <= tol1 || fb == 0) return b;       /* (the best end is returned: the ordering above ran after the last evaluation) */
        if (M_ABS(e) >= tol1 && M_ABS(fa) > M_ABS(fb)) {
            FT sq = fb / fa, pp, q;
            if (a == c) { pp = 2 * xm * sq; q = 1 - sq; }                   /* secant */
            else {                                                          /* inverse quadratic interpolation */
                FT qa = fa / fc, r = fb / fc;
                pp = sq * (2 * xm * qa * (qa - r) - (b - a) * (r - 1));
                q = (qa - 1) * (r - 1) * (sq - 1);
            }
            if (pp > 0) q = -q;
            pp = M_ABS(pp);
            if (2 * pp < FN(o_min)(3 * xm * q - M_ABS(tol1 * q), M_ABS(e * q))) { e = d; d = pp / q; }
            else { d = xm; e = d; }
        } else { d = xm; e = d; }
        a = b; fa = fb;
        b += M_ABS(d) > tol1 ? d : (xm > 0 ? tol1 : -tol1);
        fb = f(b, ctx);
    }
}

typedef struct TY(cmxo_p3_state) {
    FT rho_q_ice, rho_n_ice, F_rim, rho_rim, rho_g, D_th, D_gr, D_cr;
    FT eps;   /* eps(FT) of the float type whose gates are being evaluated */
} TY(cmxo_p3_state);

/* UT.gamma_inc — src/Utilities.jl:93-144: (P, Q) with a fixed number of series / Lentz iterations */
static inline void FN(o_gamma_inc)(FT a, FT x, int maxiters, FT *P, FT *Q) {
    if (x <= 0) { *P = 0; *Q = 1; return; }
    if (isinf(x)) { *P = 1; *Q = 0; return; }
    FT factor = M_EXP(a * M_LOG(x) - x - M_LGAMMA(a));
    if (x < a + 1) {
        FT term = (FT)1 / a, sum = term;
        for (int k = 1; k <= maxiters; ++k) { term *= x / (a + k); sum += term; }
        FT p = FN(o_clamp)(factor * sum, (FT)0, (FT)1);
        *P = p; *Q = (FT)1 - p;
    } else {
        const FT tiny = (FT)1e-30;
        FT b1 = x + 1 - a, c = b1 + 1 / tiny, d = 1 / b1, h = d;
        for (int k = 1; k <= maxiters; ++k) {
            FT ak = -(FT)k * ((FT)k - a), bk = x + 2 * k + 1 - a;
            FT dt = bk + ak * d;
            d = M_ABS(dt) < tiny ? tiny : dt;
            FT ct = bk + ak / c;
            c = M_ABS(ct) < tiny ? tiny : ct;
            d = 1 / d;
            h *= c * d;
        }
        FT q = FN(o_clamp)(factor * h, (FT)0, (FT)1);
        *P = (FT)1 - q; *Q = q;
    }
}

/* UT.sgs_weight_function / _regularised_ratio — src/Utilities.jl:445-488 */
static inline FT FN(o_sgs_weight)(FT a, FT a_half, FT eps) {
    if (a < 0) return 0;
    if (a > FN(o_min)((FT)1, 42 * a_half)) return 1;
    if (4 * a < eps) return 0;
    return (1 + M_TANH(2 * M_ATANH(1 - 2 * M_POW(1 - a, -1 / M_LOG2(1 - a_half))))) / 2;
}
static inline FT FN(o_regularised_ratio)(FT num, FT den, FT eps) {   /* eps = eps(FT) of the gates' float type */
    FT half = eps, eps2 = eps * eps;
    FT wgt = FN(o_sgs_weight)(den, half, eps);
    return den < eps2 ? (FT)0 : wgt * num / den;
}
/* exprel — src/P3_particle_properties.jl:159-199 */
static inline FT FN(o_exprel1)(FT x) { return M_EXPM1(x) / x; }
static inline FT FN(o_exprel2)(FT x) {
    if (M_ABS(x) < (FT)(1.0 / 5)) {   /* evalpoly(x, (1/2!, …, 1/9!)) */
        static const double inv_fac[8] = {1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880};
        FT r = (FT)inv_fac[7];
        for (int i = 6; i >= 0; --i) r = r * x + (FT)inv_fac[i];
        return r;
    }
    return (M_EXPM1(x) - x) / (x * x);
}
/* get_ρ_d — :191-199 */
static inline FT FN(o_p3_rho_d)(const TY(cmx_p3_params) * pr, FT F_rim, FT rho_rim) {
    FT p = 1 / (3 - pr->beta_va);
    FT logFu = M_LOG1P(-F_rim);
    FT phi1 = FN(o_exprel1)(logFu);
    FT phi1mp = FN(o_exprel1)((1 - p) * logFu);
    FT H = -p * FN(o_exprel2)(-p * logFu) - (1 - p) * FN(o_exprel2)((1 - p) * logFu);
    FT G = H - phi1mp * phi1;
    return -(rho_rim * phi1 * phi1mp) / G;
}
static inline FT FN(o_p3_threshold)(const TY(cmx_p3_params) * pr, FT rho) {   /* :222-226 */
    return M_POW(6 * pr->alpha_va / ((FT)M_PI * rho), 1 / (3 - pr->beta_va));
}
/* P3State(params, ρq_ice, ρn_ice, F_rim, ρ_rim) — :43-56 */
static inline TY(cmxo_p3_state) FN(o_p3_state)(const TY(cmx_p3_params) * pr, FT rho_q_ice, FT rho_n_ice, FT F_rim, FT rho_rim, FT eps) {
    TY(cmxo_p3_state) s;
    s.eps = eps;
    FT rho_d = FN(o_p3_rho_d)(pr, F_rim, rho_rim);
    s.rho_q_ice = rho_q_ice; s.rho_n_ice = rho_n_ice; s.F_rim = F_rim; s.rho_rim = rho_rim;
    s.rho_g = F_rim * rho_rim + (1 - F_rim) * rho_d;                         /* weighted_average :293-295 */
    s.D_th = FN(o_p3_threshold)(pr, pr->rho_i);
    s.D_gr = (F_rim == 0) ? (FT)INFINITY : FN(o_p3_threshold)(pr, s.rho_g);
    s.D_cr = (F_rim == 0) ? (FT)INFINITY : FN(o_p3_threshold)(pr, s.rho_g * (1 - F_rim));
    return s;
}
/* state_from_prognostic — :101-106 */
static inline TY(cmxo_p3_state) FN(o_p3_state_from_prognostic)(const TY(cmx_p3_params) * pr, FT rho_q_ice, FT rho_n_ice,
                                                              FT rho_q_rim, FT rho_b_rim, FT eps) {
    FT F_rim = FN(o_min)(FN(o_regularised_ratio)(FN(o_min)(rho_q_rim, rho_q_ice), rho_q_ice, eps), (FT)1 - eps);
    FT rho_rim = FN(o_min)(FN(o_regularised_ratio)(rho_q_rim, rho_b_rim, eps), (FT)0.8 * pr->rho_l);
    return FN(o_p3_state)(pr, rho_q_ice, rho_n_ice, F_rim, rho_rim, eps);
}
/* ice_mass_coeffs at D — :346-356 with regime_value :320-332 */
static inline void FN(o_p3_mass_coeffs)(const TY(cmx_p3_params) * pr, const TY(cmxo_p3_state) * s, FT D, FT *a, FT *b) {
    const FT pi = (FT)M_PI;
    FT Fu = FN(o_max)(1 - s->F_rim, s->eps);
    if (D < s->D_th) { *a = pr->rho_i * pi / 6; *b = 3; }
    else if (s->F_rim == 0) { *a = pr->alpha_va; *b = pr->beta_va; }
    else if (D < s->D_gr) { *a = pr->alpha_va; *b = pr->beta_va; }
    else if (D < s->D_cr) { *a = s->rho_g * pi / 6; *b = 3; }
    else { *a = pr->alpha_va / Fu; *b = pr->beta_va; }
}
/* get_μ — :171-173 */
static inline FT FN(o_p3_mu)(const TY(cmx_p3_params) * pr, uint32_t flags, FT loglam) {
    if (flags & CMX_P3_SLOPE_CONSTANT) return pr->mu_const;
    return FN(o_clamp)(pr->slope_a * M_POW(M_EXP(loglam), pr->slope_b) - pr->slope_c, (FT)0, pr->mu_max);
}
/* loggamma_inc_moment — :97-109 */
static inline FT FN(o_loggamma_inc_moment)(FT D1, FT D2, FT mu, FT loglam, FT k, FT scale, int gi_iters, FT eps) {
    if (!(D1 < D2)) return -(FT)INFINITY;
    FT z = k + mu + 1;
    FT x1 = D1 * M_EXP(loglam), x2 = D2 * M_EXP(loglam);
    FT p1, q1, p2, q2;
    FN(o_gamma_inc)(z, x1, gi_iters, &p1, &q1);
    FN(o_gamma_inc)(z, x2, gi_iters, &p2, &q2);
    FT dq = x2 < z + 1 ? p2 - p1 : q1 - q2;
    dq = FN(o_max)(dq, eps);
    return -z * loglam + M_LGAMMA(z) + M_LOG(dq) + M_LOG(scale);
}
/* UT.unrolled_logsumexp — src/Utilities.jl:399-412: the maximum with Julia's NaN rule (any NaN element makes it NaN), returned as it is when
 * not finite (+Inf, −Inf, NaN: no Inf − Inf below), else max + log Σ exp(x_i − max) */
static inline FT FN(o_unrolled_logsumexp)(const FT *x, int n) {
    FT xmax = -(FT)INFINITY;
    for (int i = 0; i < n; ++i) {
        if (isnan(x[i])) xmax = x[i];
        else if (!isnan(xmax) && x[i] > xmax) xmax = x[i];
    }
    if (!isfinite(xmax)) return xmax;
    FT sum = 0;
    for (int i = 0; i < n; ++i) sum += M_EXP(x[i] - xmax);
    return xmax + M_LOG(sum);
}
/* logmass_gamma_moment — :193-200 (4 segments + unrolled_logsumexp) */
static inline FT FN(o_logmass_gamma_moment)(const TY(cmx_p3_params) * pr, const TY(cmxo_p3_state) * s, FT mu, FT loglam,
                                           FT n, int gi_iters) {
    FT bnd[5] = {0, s->D_th, s->D_gr, s->D_cr, (FT)INFINITY};
    FT m[4];
    for (int i = 0; i < 4; ++i) {
        FT a, b;
        FN(o_p3_mass_coeffs)(pr, s, (bnd[i] + bnd[i + 1]) / 2, &a, &b);
        m[i] = FN(o_loggamma_inc_moment)(bnd[i], bnd[i + 1], mu, loglam, b + n, a, gi_iters, s->eps);
    }
    return FN(o_unrolled_logsumexp)(m, 4);
}
static inline FT FN(o_loggamma_moment)(FT mu, FT loglam, FT k) {   /* :151-157, scale = 1 */
    FT z = k + mu + 1;
    return -z * loglam + M_LGAMMA(z);
}
/* logLdivN — :211-216 */
static inline FT FN(o_logLdivN)(const TY(cmx_p3_params) * pr, uint32_t flags, const TY(cmxo_p3_state) * s, FT loglam, int gi_iters) {
    FT mu = FN(o_p3_mu)(pr, flags, loglam);
    return FN(o_logmass_gamma_moment)(pr, s, mu, loglam, (FT)0, gi_iters) - FN(o_loggamma_moment)(mu, loglam, (FT)0);
}
/* get_distribution_logλ — :284-320 with the warm-start bracket of _narrow_bracket :336-353; Brent's method on [2, 17] */
typedef struct TY(cmxo_shape_ctx) { const TY(cmx_p3_params) * pr; uint32_t flags; const TY(cmxo_p3_state) * s; FT target; int gi_iters; } TY(cmxo_shape_ctx);
static FT FN(o_shape_problem)(FT loglam, const void *ctx) {
    const TY(cmxo_shape_ctx) *k = (const TY(cmxo_shape_ctx) *)ctx;
    return FN(o_logLdivN)(k->pr, k->flags, k->s, loglam, k->gi_iters) - k->target;
}
static inline FT FN(o_p3_loglambda)(const TY(cmx_p3_params) * pr, uint32_t flags, const TY(cmxo_p3_state) * s,
                                   const TY(cmxo_thresholds) * th, int maxiters, int gi_iters, const FT *guess) {
    if (s->rho_n_ice < th->eps_n || s->rho_q_ice < th->eps_m) return -(FT)INFINITY;
    TY(cmxo_shape_ctx) k = {pr, flags, s, M_LOG(s->rho_q_ice) - M_LOG(s->rho_n_ice), gi_iters};
#define SHAPE(x) FN(o_shape_problem)((x), &k)
    FT a = 2, b = 17, fa = SHAPE(a), fb = SHAPE(b);
    if (!isfinite(fa) || !isfinite(fb) || fa * fb > 0) return M_ABS(fa) <= M_ABS(fb) ? a : b;
    if (guess) {   /* _narrow_bracket — :336-353 (a = lo, b = hi at this point) */
        FT pg = *guess;
        int valid = isfinite(pg) && (a < pg && pg < b);
        FT pc = valid ? pg : a;
        FT fp = SHAPE(pc);
        valid = valid && isfinite(fp);
        int left = valid && (fa * fp < 0);
        int right = valid && !left;
        if (left) { b = pc; fb = fp; }
        if (right) { a = pc; fa = fp; }
    }
#undef SHAPE
    return FN(o_brent_fixed)(FN(o_shape_problem), &k, a, b, fa, fb, maxiters);
}
/* D_m — src/P3_integral_properties.jl:56-61 */
static inline FT FN(o_p3_D_m)(const TY(cmx_p3_params) * pr, uint32_t flags, const TY(cmxo_p3_state) * s, FT loglam, int gi_iters) {
    FT mu = FN(o_p3_mu)(pr, flags, loglam);
    FT mwm = FN(o_logmass_gamma_moment)(pr, s, mu, loglam, (FT)1, gi_iters);
    FT logN0 = M_LOG(s->rho_n_ice) - FN(o_loggamma_moment)(mu, loglam, (FT)0);   /* get_logN₀ :233-237 */
    return M_EXP(logN0 + mwm) / s->rho_q_ice;
}

/* oracle twin of cmx_p3_shape_*: columns x3, x4 are (ρq_rim, ρb_rim) or, with CMX_P3_INPUT_IS_STATE, (F_rim, ρ_rim).
 * maxiters ≤ 0 → the reference's fixed budget (8 Float32 / 10 Float64); gi_iters ≤ 0 → 20 / 30. */
void FN(cmxo_p3_shape)(const TY(cmx_p3_params) * pr, uint32_t flags, const TY(cmxo_thresholds) * th, int maxiters, int gi_iters,
                      int64_t n, const FT *rho_q_ice, const FT *rho_n_ice, const FT *x3, const FT *x4, const FT *guess,
                      FT *F_rim, FT *rho_rim, FT *rho_g, FT *D_gr, FT *D_cr, FT *loglam, FT *D_m, FT *logN0, int32_t nthreads) {
    if (maxiters <= 0) maxiters = sizeof(FT) == 4 ? 8 : 10;
    if (gi_iters <= 0) gi_iters = sizeof(FT) == 4 ? 20 : 30;
    (void)nthreads;
#pragma omp parallel for schedule(dynamic, 64) num_threads(nthreads > 0 ? nthreads : 1)
    for (int64_t i = 0; i < n; ++i) {
        TY(cmxo_p3_state) s = (flags & CMX_P3_INPUT_IS_STATE) ? FN(o_p3_state)(pr, rho_q_ice[i], rho_n_ice[i], x3[i], x4[i], th->eps_ft)
                                                              : FN(o_p3_state_from_prognostic)(pr, rho_q_ice[i], rho_n_ice[i], x3[i], x4[i], th->eps_ft);
        FT ll = FN(o_p3_loglambda)(pr, flags, &s, th, maxiters, gi_iters, guess ? &guess[i] : NULL);
        if (F_rim) F_rim[i] = s.F_rim;
        if (rho_rim) rho_rim[i] = s.rho_rim;
        if (rho_g) rho_g[i] = s.rho_g;
        if (D_gr) D_gr[i] = s.D_gr;
        if (D_cr) D_cr[i] = s.D_cr;
        if (loglam) loglam[i] = ll;
        if (D_m) D_m[i] = FN(o_p3_D_m)(pr, flags, &s, ll, gi_iters);
        if (logN0) logN0[i] = M_LOG(s.rho_n_ice) - FN(o_loggamma_moment)(FN(o_p3_mu)(pr, flags, ll), ll, (FT)0);
    }
}
/* ---- weighted fall speeds: src/P3_terminal_velocity.jl, src/P3_integral_properties.jl:34-46 ------------------- */
/* UT._gamma_inc_inv — src/Utilities.jl:205-252 (Halley, ≤15 iterations; eps = eps(FT) of the gates) */
static inline FT FN(o_gamma_inc_inv)(FT a, FT p, FT q, int gi_iters, FT eps) {
    if (p <= 0) return 0;
    if (q <= 0) return (FT)INFINITY;
    FT x = (p < (FT)0.5) ? M_POW(p * M_TGAMMA(a + 1), 1 / a) : a - M_LOG(q);
    int use_q = p > (FT)0.5;
    FT lg = M_LGAMMA(a);
    for (int i = 0; i < 15; ++i) {
        FT P, Q;
        FN(o_gamma_inc)(a, x, gi_iters, &P, &Q);
        FT f = use_q ? Q - q : P - p;
        FT fprime = M_EXP((a - 1) * M_LOG(x) - x - lg);
        if (use_q) fprime = -fprime;
        if (fprime == 0) break;
        FT r = (a - 1 - x) / x;
        FT step = f / (fprime * (1 - (FT)0.5 * f * r / fprime));
        if (x - step <= 0) step = (FT)0.5 * x;
        x = x - step;
        if (M_ABS(step) < eps * x) break;
    }
    return x;
}
/* CO.Chen2022_vel_coeffs (small / large ice) — src/Common.jl:304-350; k = 0, 1 */
static inline void FN(o_chen_small_ice)(const TY(cmx_chen2022_small_ice_vel) * c, FT rho_a, FT rho_i, FT ai[2], FT bi[2], FT ci[2]) {
    rho_a = FN(o_max)(rho_a, (FT)0);
    FT l = M_LOG(rho_i), sq = M_SQRT(rho_i);
    FT As = c->A[1] * l * l - c->A[2] * l + c->A[0];
    FT Bs = 1 / (c->B[0] + c->B[1] * l + c->B[2] / sq);
    FT Cs = c->C[0] + c->C[1] * M_EXP(c->C[2] * rho_i) + c->C[3] * sq;
    FT Es = c->E[0] - c->E[1] * l * l + c->E[2] * sq;
    FT Fs = -M_EXP(c->F[0] - c->F[1] * l * l + c->F[2] * l);
    FT Gs = 1 / (c->G[0] + c->G[1] / l - c->G[2] * l / rho_i);
    FT ra = M_POW(rho_a, As);
    bi[0] = bi[1] = Bs + rho_a * Cs;
    ai[0] = Es * ra * M_POW((FT)1000, bi[0]); ai[1] = Fs * ra * M_POW((FT)1000, bi[1]);
    ci[0] = 0; ci[1] = Gs * 1000;
}
static inline void FN(o_chen_large_ice)(const TY(cmx_chen2022_large_ice_vel) * c, FT rho_a, FT rho_i, FT ai[2], FT bi[2], FT ci[2]) {
    rho_a = FN(o_max)(rho_a, (FT)0);
    FT l = M_LOG(rho_i), sq = M_SQRT(rho_i);
    FT Al = c->A[0] + c->A[1] * l + c->A[2] / (rho_i * sq);
    FT Bl = M_EXP(c->B[0] + c->B[1] * l * l + c->B[2] * l);
    FT Cl = M_EXP(c->C[0] + c->C[1] / l + c->C[2] / rho_i);
    FT El = c->E[0] + c->E[1] * l * sq + c->E[2] * sq;
    FT Fl = c->F[0] + c->F[1] * l - M_EXP(M_LOG(-c->F[2]) - rho_i);
    FT Gl = 1 / (c->G[0] + c->G[1] * l * sq + c->G[2] / sq);
    FT Hl = c->H[0] + c->H[1] * rho_i * rho_i * sq + M_EXP(M_LOG(-c->H[2]) - rho_i);
    FT ra = M_POW(rho_a, Al);
    bi[0] = Cl; bi[1] = Fl;
    ai[0] = Bl * ra * M_POW((FT)1000, bi[0]); ai[1] = El * ra * M_EXP(Hl * rho_a) * M_POW((FT)1000, bi[1]);
    ci[0] = 0; ci[1] = Gl * 1000;
}
/* regime_value — src/P3_particle_properties.jl:320-332 */
static inline FT FN(o_p3_regime)(const TY(cmxo_p3_state) * s, FT D, FT small, FT unrimed, FT dense, FT graupel, FT partial) {
    return D < s->D_th ? small : (s->F_rim == 0 ? unrimed : (D < s->D_gr ? dense : (D < s->D_cr ? graupel : partial)));
}
static inline FT FN(o_p3_ice_mass)(const TY(cmx_p3_params) * pr, const TY(cmxo_p3_state) * s, FT D) {   /* :366-369 */
    FT a, b;
    FN(o_p3_mass_coeffs)(pr, s, D, &a, &b);
    return a * M_POW(D, b);
}
static inline FT FN(o_p3_ice_area)(const TY(cmx_p3_params) * pr, const TY(cmxo_p3_state) * s, FT D) {   /* :412-421 */
    FT sph = D * D * (FT)M_PI / 4, non = pr->gamma * M_POW(D, pr->sigma);
    return FN(o_p3_regime)(s, D, sph, non, non, sph, s->F_rim * sph + (1 - s->F_rim) * non);
}
static inline FT FN(o_p3_phi)(const TY(cmx_p3_params) * pr, const TY(cmxo_p3_state) * s, FT D) {   /* ϕᵢ :462-475 */
    FT m = FN(o_p3_ice_mass)(pr, s, D), a = FN(o_p3_ice_area)(pr, s, D);
    FT rho = FN(o_p3_regime)(s, D, pr->rho_i, pr->rho_i, pr->rho_i, s->rho_g, pr->rho_i);
    FT phi = 3 * M_SQRT((FT)M_PI) * m / (4 * rho * a * M_SQRT(a));
    return D == 0 ? (FT)0 : phi;
}
typedef struct TY(cmxo_p3_vterm) { FT as[2], bs[2], cs[2], al[2], bl[2], cl[2], cutoff; int aspect; } TY(cmxo_p3_vterm);
/* P3IceParticleVelocityFunctor — src/P3_terminal_velocity.jl:11-21; Chen2022VelocityCurve src/Common.jl:381-382 */
static inline FT FN(o_p3_particle_velocity)(const TY(cmx_p3_params) * pr, const TY(cmxo_p3_state) * s, const TY(cmxo_p3_vterm) * v, FT D) {
    FT vs = v->as[0] * M_POW(D, v->bs[0]) * M_EXP(-v->cs[0] * D) + v->as[1] * M_POW(D, v->bs[1]) * M_EXP(-v->cs[1] * D);
    FT vl = v->al[0] * M_POW(D, v->bl[0]) * M_EXP(-v->cl[0] * D) + v->al[1] * M_POW(D, v->bl[1]) * M_EXP(-v->cl[1] * D);
    FT vt = D <= v->cutoff ? vs : vl;
    return vt * (v->aspect ? M_CBRT(FN(o_p3_phi)(pr, s, D)) : (FT)1);
}
/* ice_terminal_velocity_{number,mass}_weighted — src/P3_terminal_velocity.jl:72-91,118-137 with integral_bounds
 * (src/P3_integral_properties.jl:34-46), segment_boundaries (src/P3_particle_properties.jl:287-292) and
 * Quadrature.integrate (src/Quadrature.jl:62-125). */
static inline void FN(o_p3_velocities)(const TY(cmx_p3_params) * pr, const TY(cmx_chen2022_ice_vel) * vel, const TY(cmx_quadrature) * quad,
                                      uint32_t flags, const TY(cmxo_p3_state) * s, FT rho_a, FT loglam, FT p, int gi_iters, FT *v_n, FT *v_m) {
    if (s->rho_n_ice < s->eps || s->rho_q_ice < s->eps) { *v_n = 0; *v_m = 0; return; }
    TY(cmxo_p3_vterm) vt;
    const FT rho_i = (FT)916.7;
    FN(o_chen_small_ice)(&vel->small_ice, rho_a, rho_i, vt.as, vt.bs, vt.cs);
    FN(o_chen_large_ice)(&vel->large_ice, rho_a, rho_i, vt.al, vt.bl, vt.cl);
    vt.cutoff = vel->small_ice.cutoff;
    vt.aspect = !(flags & CMX_P3_NO_ASPECT_RATIO);
    FT mu = FN(o_p3_mu)(pr, flags, loglam), lam = M_EXP(loglam);
    FT logN0 = M_LOG(s->rho_n_ice) - FN(o_loggamma_moment)(mu, loglam, (FT)0);
    FT Y1 = p, Y2 = (FT)(1.0 - (double)p);   /* FT(p), FT(1 - p) with p a Float64 keyword in the reference */
    FT Q1 = 1 - Y1, Q2 = 1 - Y2;
    if (s->eps > (FT)1e-10) {   /* Float32 gates: the quantile levels are Float32 numbers (1 − Float32(1−1e-6) = 1.0133e-6) */
        Y1 = (FT)(float)Y1; Y2 = (FT)(float)(1.0 - (double)p);
        Q1 = (FT)(1.0f - (float)Y1); Q2 = (FT)(1.0f - (float)Y2);
    }
    FT D_min = FN(o_gamma_inc_inv)(mu + 1, Y1, Q1, gi_iters, s->eps) / lam;
    FT D_max = FN(o_gamma_inc_inv)(mu + 1, Y2, Q2, gi_iters, s->eps) / lam;
    FT bnd[5] = {D_min, FN(o_clamp)(s->D_th, D_min, D_max), FN(o_clamp)(s->D_gr, D_min, D_max), FN(o_clamp)(s->D_cr, D_min, D_max), D_max};
    FT sum_n = 0, sum_m = 0;
    for (int k = 0; k < 4; ++k) {
        FT a = bnd[k], b = bnd[k + 1];
        if (!(a < b)) continue;
        FT scale = (b - a) / 2, shift = (a + b) / 2, rn = 0, rm = 0;
        for (int i = 0; i < Q_N(quad); ++i) {
            FT x = scale * Q_NODE(quad, i) + shift, w = Q_WEIGHT(quad, i);
            FT nD = M_EXP(logN0 + mu * M_LOG(x) - lam * x);
            FT nv = nD * FN(o_p3_particle_velocity)(pr, s, &vt, x);
            rn += nv * w;
            rm += nv * FN(o_p3_ice_mass)(pr, s, x) * w;
        }
        sum_n += scale * rn; sum_m += scale * rm;
    }
    *v_n = sum_n / s->rho_n_ice; *v_m = sum_m / s->rho_q_ice;
}
void FN(cmxo_p3_terminal_velocities)(const TY(cmx_p3_params) * pr, const TY(cmx_chen2022_ice_vel) * vel, const TY(cmx_quadrature) * quad,
                                    uint32_t flags, const TY(cmxo_thresholds) * th, int gi_iters, FT p, int64_t n, const FT *rho_q_ice,
                                    const FT *rho_n_ice, const FT *x3, const FT *x4, const FT *rho_a, const FT *loglam, FT *v_n, FT *v_m,
                                    int32_t nthreads) {
    if (gi_iters <= 0) gi_iters = sizeof(FT) == 4 ? 20 : 30;
    (void)nthreads;
#pragma omp parallel for schedule(dynamic, 16) num_threads(nthreads > 0 ? nthreads : 1)
    for (int64_t i = 0; i < n; ++i) {
        TY(cmxo_p3_state) s = (flags & CMX_P3_INPUT_IS_STATE) ? FN(o_p3_state)(pr, rho_q_ice[i], rho_n_ice[i], x3[i], x4[i], th->eps_ft)
                                                              : FN(o_p3_state_from_prognostic)(pr, rho_q_ice[i], rho_n_ice[i], x3[i], x4[i], th->eps_ft);
        FN(o_p3_velocities)(pr, vel, quad, flags, &s, rho_a[i], loglam[i], p, gi_iters, &v_n[i], &v_m[i]);
    }
}
/* CO.ventilation_factor — src/Common.jl:506-514: F_v(D) = a_v + b_v ∛N_Sc √N_Re(D), N_Sc = ν/D_v, N_Re = D v_term(D)/ν */
static inline FT FN(o_ventilation_factor)(const TY(cmx_ventilation) * vent, const TY(cmx_air_properties) * aps, FT cbrt_Nsc, FT D, FT v_term) {
    return vent->a + vent->b * cbrt_Nsc * M_SQRT(D * v_term / aps->nu_air);
}
/* ice_melt — src/P3_processes.jl:64-94 (QIMLT of Morrison & Milbrandt 2015): dL/dt = 4 K/L_f (T − T_freeze) ∫ ∂m/∂D F_v(D) N′(D)/D dD
 * with the ventilation factor CO.ventilation_factor (src/Common.jl:506-514); dN/dt = N/L · dL/dt. */
static inline void FN(o_p3_ice_melt)(const TY(cmx_p3_params) * pr, const TY(cmx_chen2022_ice_vel) * vel, const TY(cmx_air_properties) * aps,
                                    const TY(cmx_thermo) * tps, const TY(cmx_ventilation) * vent, const TY(cmx_quadrature) * quad,
                                    uint32_t flags, const TY(cmxo_p3_state) * s, FT rho_a, FT T, FT loglam, FT p, int gi_iters,
                                    FT *dNdt, FT *dLdt) {
    if (s->rho_n_ice < s->eps || s->rho_q_ice < s->eps) { *dNdt = 0; *dLdt = 0; return; }   /* N/L undefined: no ice, no melt */
    TY(cmxo_p3_vterm) vt;
    const FT rho_i = (FT)916.7;
    FN(o_chen_small_ice)(&vel->small_ice, rho_a, rho_i, vt.as, vt.bs, vt.cs);
    FN(o_chen_large_ice)(&vel->large_ice, rho_a, rho_i, vt.al, vt.bl, vt.cl);
    vt.cutoff = vel->small_ice.cutoff;
    vt.aspect = !(flags & CMX_P3_NO_ASPECT_RATIO);
    FT mu = FN(o_p3_mu)(pr, flags, loglam), lam = M_EXP(loglam);
    FT logN0 = M_LOG(s->rho_n_ice) - FN(o_loggamma_moment)(mu, loglam, (FT)0);
    FT Y1 = p, Y2 = (FT)(1.0 - (double)p), Q1 = 1 - Y1, Q2 = 1 - Y2;
    if (s->eps > (FT)1e-10) {
        Y1 = (FT)(float)Y1; Y2 = (FT)(float)(1.0 - (double)p);
        Q1 = (FT)(1.0f - (float)Y1); Q2 = (FT)(1.0f - (float)Y2);
    }
    FT D_min = FN(o_gamma_inc_inv)(mu + 1, Y1, Q1, gi_iters, s->eps) / lam;
    FT D_max = FN(o_gamma_inc_inv)(mu + 1, Y2, Q2, gi_iters, s->eps) / lam;
    FT bnd[5] = {D_min, FN(o_clamp)(s->D_th, D_min, D_max), FN(o_clamp)(s->D_gr, D_min, D_max), FN(o_clamp)(s->D_cr, D_min, D_max), D_max};
    FT cbrt_Nsc = M_CBRT(aps->nu_air / aps->D_vapor);
    FT total = 0;
    for (int k = 0; k < 4; ++k) {
        FT a = bnd[k], b = bnd[k + 1];
        if (!(a < b)) continue;
        FT scale = (b - a) / 2, shift = (a + b) / 2, r = 0;
        for (int i = 0; i < Q_N(quad); ++i) {
            FT x = scale * Q_NODE(quad, i) + shift, w = Q_WEIGHT(quad, i);
            FT nD = M_EXP(logN0 + mu * M_LOG(x) - lam * x);
            FT ma, mb;
            FN(o_p3_mass_coeffs)(pr, s, x, &ma, &mb);
            FT dm = ma * mb * M_POW(x, mb - 1);                                       /* ∂ice_mass_∂D :394-397 */
            FT Fv = FN(o_ventilation_factor)(vent, aps, cbrt_Nsc, x, FN(o_p3_particle_velocity)(pr, s, &vt, x));
            r += dm * Fv * nD / x * w;
        }
        total += scale * r;
    }
    FT L_f = FN(o_latent_heat_fusion)(tps, T);
    FT dL = FN(o_max)((FT)0, 4 * aps->K_therm / L_f * (T - pr->T_freeze) * total);
    *dLdt = dL;
    *dNdt = s->rho_n_ice / s->rho_q_ice * dL;
}
void FN(cmxo_p3_ice_melt)(const TY(cmx_p3_params) * pr, const TY(cmx_chen2022_ice_vel) * vel, const TY(cmx_air_properties) * aps,
                         const TY(cmx_thermo) * tps, const TY(cmx_ventilation) * vent, const TY(cmx_quadrature) * quad, uint32_t flags,
                         const TY(cmxo_thresholds) * th, FT p, int64_t n, const FT *rho_q_ice, const FT *rho_n_ice, const FT *x3,
                         const FT *x4, const FT *rho_a, const FT *T, const FT *loglam, FT *dNdt, FT *dLdt, int32_t nthreads) {
    const int gi_iters = sizeof(FT) == 4 ? 20 : 30;
    (void)nthreads;
#pragma omp parallel for schedule(dynamic, 16) num_threads(nthreads > 0 ? nthreads : 1)
    for (int64_t i = 0; i < n; ++i) {
        TY(cmxo_p3_state) s = (flags & CMX_P3_INPUT_IS_STATE) ? FN(o_p3_state)(pr, rho_q_ice[i], rho_n_ice[i], x3[i], x4[i], th->eps_ft)
                                                              : FN(o_p3_state_from_prognostic)(pr, rho_q_ice[i], rho_n_ice[i], x3[i], x4[i], th->eps_ft);
        FN(o_p3_ice_melt)(pr, vel, aps, tps, vent, quad, flags, &s, rho_a[i], T[i], loglam[i], p, gi_iters, &dNdt[i], &dLdt[i]);
    }
}
/* ice_self_collection — src/P3_processes.jl:676-712: dN/dt = ½ ∫∫ π (r₁+r₂)² |v₁−v₂| n(D₁) n(D₂) dD₂ dD₁, r = √(ice_area/π), E = 1;
 * outer integral over the regime segments between the eps(FT) and 1−eps(FT) quantiles, inner integral split at the cusp D₂ = D₁ */
static inline FT FN(o_p3_ice_self_collection)(const TY(cmx_p3_params) * pr, const TY(cmx_chen2022_ice_vel) * vel, const TY(cmx_quadrature) * quad,
                                             uint32_t flags, const TY(cmxo_p3_state) * s, FT rho_a, FT loglam, int gi_iters) {
    if (s->rho_n_ice < s->eps || s->rho_q_ice < s->eps) return 0;
    TY(cmxo_p3_vterm) vt;
    const FT rho_i = (FT)916.7, pi = (FT)M_PI;
    FN(o_chen_small_ice)(&vel->small_ice, rho_a, rho_i, vt.as, vt.bs, vt.cs);
    FN(o_chen_large_ice)(&vel->large_ice, rho_a, rho_i, vt.al, vt.bl, vt.cl);
    vt.cutoff = vel->small_ice.cutoff;
    vt.aspect = !(flags & CMX_P3_NO_ASPECT_RATIO);
    FT mu = FN(o_p3_mu)(pr, flags, loglam), lam = M_EXP(loglam);
    FT logN0 = M_LOG(s->rho_n_ice) - FN(o_loggamma_moment)(mu, loglam, (FT)0);
    FT Y1 = s->eps, Y2 = 1 - s->eps;            /* p = eps(one(ρₐ)) */
    FT D_lo = FN(o_gamma_inc_inv)(mu + 1, Y1, 1 - Y1, gi_iters, s->eps) / lam;
    FT D_hi = FN(o_gamma_inc_inv)(mu + 1, Y2, 1 - Y2, gi_iters, s->eps) / lam;
    FT bnd[5] = {D_lo, FN(o_clamp)(s->D_th, D_lo, D_hi), FN(o_clamp)(s->D_gr, D_lo, D_hi), FN(o_clamp)(s->D_cr, D_lo, D_hi), D_hi};
    FT total = 0;
    for (int k = 0; k < 4; ++k) {
        FT a = bnd[k], b = bnd[k + 1];
        if (!(a < b)) continue;
        FT scale = (b - a) / 2, shift = (a + b) / 2, r_out = 0;
        for (int i = 0; i < Q_N(quad); ++i) {
            FT D1 = scale * Q_NODE(quad, i) + shift;
            FT v1 = FN(o_p3_particle_velocity)(pr, s, &vt, D1);
            FT r1 = M_SQRT(FN(o_p3_ice_area)(pr, s, D1) / pi);
            FT inner = 0;
            for (int h = 0; h < 2; ++h) {
                FT ia = h == 0 ? D_lo : D1, ib = h == 0 ? D1 : D_hi;
                if (!(ia < ib)) continue;
                FT sc2 = (ib - ia) / 2, sh2 = (ia + ib) / 2, r_in = 0;
                for (int j = 0; j < Q_N(quad); ++j) {
                    FT D2 = sc2 * Q_NODE(quad, j) + sh2;
                    FT v2 = FN(o_p3_particle_velocity)(pr, s, &vt, D2);
                    FT r2 = M_SQRT(FN(o_p3_ice_area)(pr, s, D2) / pi);
                    FT K = pi * (r1 + r2) * (r1 + r2);
                    r_in += K * M_ABS(v1 - v2) * M_EXP(logN0 + mu * M_LOG(D2) - lam * D2) * Q_WEIGHT(quad, j);
                }
                inner += sc2 * r_in;
            }
            r_out += inner * M_EXP(logN0 + mu * M_LOG(D1) - lam * D1) * Q_WEIGHT(quad, i);
        }
        total += scale * r_out;
    }
    return (FT)0.5 * total;
}
void FN(cmxo_p3_ice_self_collection)(const TY(cmx_p3_params) * pr, const TY(cmx_chen2022_ice_vel) * vel, const TY(cmx_quadrature) * quad,
                                    uint32_t flags, const TY(cmxo_thresholds) * th, int64_t n, const FT *rho_q_ice, const FT *rho_n_ice,
                                    const FT *x3, const FT *x4, const FT *rho_a, const FT *loglam, FT *dNdt, int32_t nthreads) {
    const int gi_iters = sizeof(FT) == 4 ? 20 : 30;
    (void)nthreads;
#pragma omp parallel for schedule(dynamic, 4) num_threads(nthreads > 0 ? nthreads : 1)
    for (int64_t i = 0; i < n; ++i) {
        TY(cmxo_p3_state) s = (flags & CMX_P3_INPUT_IS_STATE) ? FN(o_p3_state)(pr, rho_q_ice[i], rho_n_ice[i], x3[i], x4[i], th->eps_ft)
                                                              : FN(o_p3_state_from_prognostic)(pr, rho_q_ice[i], rho_n_ice[i], x3[i], x4[i], th->eps_ft);
        dNdt[i] = FN(o_p3_ice_self_collection)(pr, vel, quad, flags, &s, rho_a[i], loglam[i], gi_iters);
    }
}
/* probes for the KATs: particle fall speed at diameter D for a state built from (F_rim, ρ_rim); gamma_inc_inv */
FT FN(cmxo_p3_particle_velocity)(const TY(cmx_p3_params) * pr, const TY(cmx_chen2022_ice_vel) * vel, uint32_t flags, FT F_rim, FT rho_rim,
                                FT rho_a, FT D) {
    TY(cmxo_p3_state) s = FN(o_p3_state)(pr, (FT)0, (FT)0, F_rim, rho_rim, M_EPS);
    TY(cmxo_p3_vterm) vt;
    FN(o_chen_small_ice)(&vel->small_ice, rho_a, (FT)916.7, vt.as, vt.bs, vt.cs);
    FN(o_chen_large_ice)(&vel->large_ice, rho_a, (FT)916.7, vt.al, vt.bl, vt.cl);
    vt.cutoff = vel->small_ice.cutoff; vt.aspect = !(flags & CMX_P3_NO_ASPECT_RATIO);
    return FN(o_p3_particle_velocity)(pr, &s, &vt, D);
}
/* the ventilation factor of an ice particle of the state (F_rim, ρ_rim) at diameter D — test/ventilation_tests.jl:8-30 */
FT FN(cmxo_p3_ventilation_factor)(const TY(cmx_p3_params) * pr, const TY(cmx_chen2022_ice_vel) * vel, const TY(cmx_air_properties) * aps,
                                 const TY(cmx_ventilation) * vent, uint32_t flags, FT F_rim, FT rho_rim, FT rho_a, FT D) {
    return FN(o_ventilation_factor)(vent, aps, M_CBRT(aps->nu_air / aps->D_vapor), D, FN(cmxo_p3_particle_velocity)(pr, vel, flags, F_rim, rho_rim, rho_a, D));
}
/* ice_mass, ice_area, ϕᵢ of the state (F_rim, ρ_rim) at diameter D, and its thresholds — test/p3_tests.jl:111-166 */
void FN(cmxo_p3_particle_properties)(const TY(cmx_p3_params) * pr, FT F_rim, FT rho_rim, FT D, FT out[7]) {
    TY(cmxo_p3_state) s = FN(o_p3_state)(pr, (FT)0, (FT)0, F_rim, rho_rim, M_EPS);
    out[0] = FN(o_p3_ice_mass)(pr, &s, D); out[1] = FN(o_p3_ice_area)(pr, &s, D); out[2] = FN(o_p3_phi)(pr, &s, D);
    out[3] = s.D_th; out[4] = s.D_gr; out[5] = s.D_cr; out[6] = s.rho_g;
}
FT FN(cmxo_unrolled_logsumexp)(int32_t n, const FT *x) { return FN(o_unrolled_logsumexp)(x, n); }
/* get_ρ_g(F_rim, ρ_rim, ρ_d) — src/P3_particle_properties.jl:219 with weighted_average :293-295 */
FT FN(cmxo_p3_rho_g)(const TY(cmx_p3_params) * pr, FT F_rim, FT rho_rim) {
    TY(cmxo_p3_state) s = FN(o_p3_state)(pr, (FT)0, (FT)0, F_rim, rho_rim, M_EPS);
    return s.rho_g;
}
FT FN(cmxo_gamma_inc_inv)(FT a, FT p, FT q) { return FN(o_gamma_inc_inv)(a, p, q, sizeof(FT) == 4 ? 20 : 30, M_EPS); }
FT FN(cmxo_p3_rho_d)(const TY(cmx_p3_params) * pr, FT F_rim, FT rho_rim) { return FN(o_p3_rho_d)(pr, F_rim, rho_rim); }
FT FN(cmxo_p3_logLdivN)(const TY(cmx_p3_params) * pr, uint32_t flags, FT F_rim, FT rho_rim, FT loglam) {
    TY(cmxo_p3_state) s = FN(o_p3_state)(pr, (FT)0, (FT)0, F_rim, rho_rim, M_EPS);
    return FN(o_logLdivN)(pr, flags, &s, loglam, sizeof(FT) == 4 ? 20 : 30);
}
void FN(cmxo_gamma_inc)(FT a, FT x, FT out[2]) { FN(o_gamma_inc)(a, x, sizeof(FT) == 4 ? 20 : 30, &out[0], &out[1]); }
