"""The P3 shape equation in high precision (mpmath, 40 digits): an independent statement of what the shape solver solves.

TEST INFRASTRUCTURE.  Nothing here is shared with the oracle (oracle/cmx_oracle_p3_impl.h) or the device (csrc/cmx_p3.hpp): the
formulas are written from the reference source, cited by file:line, with exact special functions in place of its fixed-count ones:

  src/P3_particle_properties.jl   get_ρ_d :191-199 (exprel :118-125), get_ρ_g :219 (weighted_average :303-305), _get_threshold :244,
                                  D_th / D_gr / D_cr :253-272 and P3State :43-56 (Inf thresholds for F_rim = 0), segment_boundaries
                                  :287-292, regime_value :320-332, ice_mass_coeffs :346-359
  src/P3_size_distribution.jl     loggamma_inc_moment :97-109, loggamma_moment :153-157, get_μ :171-172, logmass_gamma_moment
                                  :193-200, logLdivN :211-216, get_logN₀ :233-237, get_distribution_logλ :284-297 (gates, target,
                                  the "no sign change" return)
  src/P3_integral_properties.jl   D_m :56-61

The one numerical device of the reference that is part of the EQUATION is kept: Δq = max(Δq, eps(FT)) (:107) floors every
segment's share of the regularised incomplete gamma function at eps of the float type (2⁻⁵² or 2⁻²³), so a segment that holds next
to nothing still contributes a·λ^(−z)·Γ(z)·eps.  What is NOT kept: the 20/30-term series and continued fraction of UT.gamma_inc
(ΔP is mp.gammainc(z, x₁, x₂, regularized=True), no P/Q choice, no cancellation), libm's lgamma, Float rounding of any kind, and
the root solver (every root in [2, 17] is found by a scan and refined to 1e-25).
"""
import mpmath as mp

DPS = 40
EPS = {"f64": mp.mpf(2) ** -52, "f32": mp.mpf(2) ** -23}       # eps(FT): the Δq floor (:107), Fu floor (:352) and the absent-ice gates (:286-289)
LOGLAM_MIN, LOGLAM_MAX = mp.mpf(2), mp.mpf(17)                  # get_distribution_logλ's default bracket (:284)
PARAM_NAMES = ("alpha_va", "beta_va", "rho_i", "slope_a", "slope_b", "slope_c", "mu_max", "mu_const")
mp.mp.dps = DPS


def params_from(c):
    """The fields of a ParametersP3 struct (or a dict) that the shape equation reads, as exact mpf of the given floats."""
    get = (lambda k: c[k]) if isinstance(c, dict) else (lambda k: getattr(c, k))
    return {k: mp.mpf(float(get(k))) for k in PARAM_NAMES}


def _exprel1(x):                                                # :118
    return mp.expm1(x) / x


def _exprel2(x):                                                # :119-125 — (eˣ − 1 − x)/x², in enough digits that no series is needed
    return (mp.expm1(x) - x) / (x * x)


class State:
    __slots__ = ("params", "slope", "F_rim", "rho_rim", "rho_g", "D_th", "D_gr", "D_cr", "segments")


def state(params, F_rim, rho_rim, slope="powerlaw", eps=EPS["f64"]):
    """ρ_g, the thresholds and the mass-law segments [(D_lo, D_hi, a, b)] of P3State(params, ·, ·, F_rim, ρ_rim).
    `eps` only enters Fu = max(1 − F_rim, eps) (:352), which is inert for every F_rim ≤ 1 − 2⁻²³."""
    assert slope in ("powerlaw", "constant")
    F, rr = mp.mpf(float(F_rim)), mp.mpf(float(rho_rim))
    assert 0 <= F < 1
    s = State()
    s.params, s.slope, s.F_rim, s.rho_rim = params, slope, F, rr
    al, be, rho_i = params["alpha_va"], params["beta_va"], params["rho_i"]
    thr = lambda rho: (6 * al / (mp.pi * rho)) ** (1 / (3 - be))   # noqa: E731 — :244
    with mp.workdps(2 * DPS + 20):                               # the exprel forms cancel like x² at small F_rim
        s.D_th = +thr(rho_i)                                      # :253
        if F == 0:                                                # :49-50; ρ_g is NaN in the reference and never read
            s.rho_g, s.D_gr, s.D_cr = mp.nan, mp.inf, mp.inf
        else:
            p = 1 / (3 - be)                                      # :192-198
            lFu = mp.log1p(-F)
            phi1, phi1mp = _exprel1(lFu), _exprel1((1 - p) * lFu)
            H = -p * _exprel2(-p * lFu) - (1 - p) * _exprel2((1 - p) * lFu)
            rho_d = -(rr * phi1 * phi1mp) / (H - phi1mp * phi1)
            s.rho_g = F * rr + (1 - F) * rho_d                    # :219, :303-305
            s.D_gr = +thr(s.rho_g)                                # :263
            s.D_cr = +thr(s.rho_g * (1 - F))                      # :272
    s.rho_g, s.D_gr, s.D_cr = +s.rho_g, +s.D_gr, +s.D_cr          # rounded to DPS: constants of the equation from here on
    Fu = max(1 - F, eps)                                          # :352
    bnds = (mp.mpf(0), s.D_th, s.D_gr, s.D_cr, mp.inf)           # :287-292 with D_min = 0, D_max = Inf
    s.segments = []
    for lo, hi in zip(bnds[:-1], bnds[1:]):                       # :195-198: the law of a segment is the law at its midpoint
        if not lo < hi:
            continue                                              # :99 — log(0), drops out of the logsumexp
        D = (lo + hi) / 2
        if D < s.D_th:                                            # :325-330, :355-356
            a, b = rho_i * mp.pi / 6, mp.mpf(3)
        elif F == 0 or D < s.D_gr:
            a, b = al, be
        elif D < s.D_cr:
            a, b = s.rho_g * mp.pi / 6, mp.mpf(3)
        else:
            a, b = al / Fu, be
        s.segments.append((lo, hi, a, b))
    return s


def mu_of(st, loglam):                                            # :171-172
    p = st.params
    if st.slope == "constant":
        return p["mu_const"]
    return min(max(p["slope_a"] * mp.exp(loglam) ** p["slope_b"] - p["slope_c"], 0), p["mu_max"])


def segment_terms(st, mu, loglam, n=0):
    """[(log(a λ^(−z) Γ(z)), ΔP)] per segment, z = b + n + μ + 1, ΔP the exact share of the regularised gamma function (:97-108 before the floor)."""
    lam = mp.exp(loglam)
    out = []
    for lo, hi, a, b in st.segments:
        z = b + n + mu + 1
        dP = mp.gammainc(z, lo * lam, mp.inf if hi == mp.inf else hi * lam, regularized=True)
        out.append((mp.log(a) - z * loglam + mp.loggamma(z), dP))
    return out


def _logsumexp_floored(terms, eps):
    vals = [lp + mp.log(max(dP, eps)) for lp, dP in terms]       # :107-108
    m = max(vals)
    return m + mp.log(mp.fsum(mp.exp(v - m) for v in vals))


def log_mass_moment(st, loglam, eps, n=0):                        # logmass_gamma_moment :193-200
    return _logsumexp_floored(segment_terms(st, mu_of(st, loglam), loglam, n), eps)


def _log_number_moment(mu, loglam):                               # loggamma_moment(μ, logλ; k = 0) :153-157
    return -(mu + 1) * loglam + mp.loggamma(mu + 1)


def logLdivN(st, loglam, eps):                                    # :211-216
    loglam = mp.mpf(loglam)
    return log_mass_moment(st, loglam, eps, 0) - _log_number_moment(mu_of(st, loglam), loglam)


def target(L, N):                                                 # :290
    return mp.log(mp.mpf(float(L))) - mp.log(mp.mpf(float(N)))


def residual(st, L, N, loglam, eps):
    """shape_problem(logλ) = logLdivN(state, logλ) − log(L/N) (:292)."""
    return logLdivN(st, loglam, eps) - target(L, N)


def has_ice(L, N, eps):                                           # :286-289
    return not (float(N) < eps or float(L) < eps)


def log_N0(st, N, loglam):                                        # get_logN₀ :233-237
    loglam = mp.mpf(loglam)
    return mp.log(mp.mpf(float(N))) - _log_number_moment(mu_of(st, loglam), loglam)


def D_m(st, L, N, loglam, eps):                                   # :56-61: exp(log N₀ + (n = 1 moment)) / L
    loglam = mp.mpf(loglam)
    return mp.exp(log_N0(st, N, loglam) + log_mass_moment(st, loglam, eps, 1)) / mp.mpf(float(L))


def derivatives(st, L, N, loglam, eps):
    """(∂f/∂logλ, ∂ln D_m/∂logλ, ∂log N₀/∂logλ) at fixed L, N — none depends on L or N."""
    x = mp.mpf(loglam)
    df = mp.diff(lambda y: logLdivN(st, y, eps), x)
    s = mp.diff(lambda y: log_mass_moment(st, y, eps, 1) - _log_number_moment(mu_of(st, y), y), x)
    t = mp.diff(lambda y: -_log_number_moment(mu_of(st, y), y), x)
    return df, s, t


# ---- all roots on [2, 17] -------------------------------------------------------------------------------------------------------
def scan(st, spacing=mp.mpf("0.05")):
    """(grid, per-point segment terms, per-point number moment): one pass serves both eps values and every target."""
    n = int(mp.ceil((LOGLAM_MAX - LOGLAM_MIN) / spacing))
    xs = [LOGLAM_MIN + (LOGLAM_MAX - LOGLAM_MIN) * i / n for i in range(n + 1)]
    terms, m0 = [], []
    for x in xs:
        mu = mu_of(st, x)
        terms.append(segment_terms(st, mu, x, 0))
        m0.append(_log_number_moment(mu, x))
    return xs, terms, m0


def profile(sc, eps):
    """logLdivN on the scan's grid for one eps."""
    xs, terms, m0 = sc
    return [_logsumexp_floored(t, eps) - m for t, m in zip(terms, m0)]


def refine(f, a, b, fa, fb, xtol=mp.mpf(10) ** -25):
    """The root of f in the bracket [a, b] (fa·fb < 0): Illinois false position, bisecting whenever the bracket fails to halve."""
    side = 0
    for _ in range(400):
        if abs(b - a) <= xtol:
            break
        w = b - a
        x = (a * fb - b * fa) / (fb - fa)
        if not (min(a, b) < x < max(a, b)):
            x = (a + b) / 2
        for attempt in (0, 1):
            fx = f(x)
            if fx == 0:
                return x
            if (fx > 0) == (fb > 0):
                b, fb = x, fx
                if side == -1:
                    fa /= 2
                side = -1
            else:
                a, fa = x, fx
                if side == 1:
                    fb /= 2
                side = 1
            if attempt or abs(b - a) <= w / 2:
                break
            x, side = (a + b) / 2, 0
    return (a + b) / 2


def _touching_extremum(f, a, b, sign):
    """Golden-section search on [a, b] for the extremum of f that approaches zero from `sign`; returns a point where f has the
    other sign as soon as one is seen, else None (the extremum does not reach zero)."""
    g = (mp.sqrt(5) - 1) / 2
    h = lambda x: sign * f(x)                                     # noqa: E731 — minimise h > 0
    c, d = b - g * (b - a), a + g * (b - a)
    hc, hd = h(c), h(d)
    while True:
        if hc < 0:
            return c
        if hd < 0:
            return d
        if b - a < mp.mpf(10) ** -18:
            return None
        if hc < hd:
            b, d, hd = d, c, hc
            c = b - g * (b - a)
            hc = h(c)
        else:
            a, c, hc = c, d, hd
            d = a + g * (b - a)
            hd = h(d)


def roots(st, L, N, eps, sc=None, near=mp.mpf("0.02")):
    """Every root of the residual on [2, 17] for one eps, ascending; or, where f(2)·f(17) > 0, the reference's return (:295-297):
    {"end": 2 or 17, "sign_lo": ±1, "sign_hi": ±1}.  A pair of roots between two grid points (a fold end that just reaches the
    target) is found from the sampled local extrema: wherever |f| has a local minimum below `near` without a sign change, the
    extremum is searched (slopes inside the fold are below 0.4, so 0.02 covers a 0.05 grid)."""
    sc = sc or scan(st)
    t = target(L, N)
    xs = sc[0]
    fs = [g - t for g in profile(sc, eps)]
    f = lambda x: logLdivN(st, x, eps) - t                        # noqa: E731
    if fs[0] * fs[-1] > 0:
        return {"end": 2 if abs(fs[0]) <= abs(fs[-1]) else 17, "sign_lo": int(mp.sign(fs[0])), "sign_hi": int(mp.sign(fs[-1]))}
    brackets = []
    for i in range(len(xs) - 1):
        if fs[i] == 0:
            brackets.append((xs[i], xs[i], fs[i], fs[i]))
        elif fs[i] * fs[i + 1] < 0:
            brackets.append((xs[i], xs[i + 1], fs[i], fs[i + 1]))
    for i in range(1, len(xs) - 1):
        sg = mp.sign(fs[i])
        if sg != 0 and mp.sign(fs[i - 1]) == sg == mp.sign(fs[i + 1]) and abs(fs[i]) <= min(abs(fs[i - 1]), abs(fs[i + 1])) and abs(fs[i]) < near:
            x = _touching_extremum(f, xs[i - 1], xs[i + 1], sg)
            if x is not None:
                fx = f(x)
                brackets += [(xs[i - 1], x, fs[i - 1], fx), (x, xs[i + 1], fx, fs[i + 1])]
    out = sorted(a if a == b else refine(f, a, b, fa, fb) for a, b, fa, fb in brackets)
    return {"roots": out}


def extrema(st, eps, lo=8, hi=11, sc=None):
    """Interior local extrema [(logλ, logLdivN, 'min' | 'max')] of logLdivN between lo and hi, located to 1e-18 (the generator
    draws its fold and fold-edge targets from them)."""
    sc = sc or scan(st)
    xs, gs = sc[0], profile(sc, eps)
    f = lambda x: logLdivN(st, x, eps)                            # noqa: E731
    out = []
    for i in range(1, len(xs) - 1):
        if not (lo <= xs[i] <= hi):
            continue
        for kind, sg in (("max", -1), ("min", 1)):
            if sg * gs[i] <= sg * gs[i - 1] and sg * gs[i] < sg * gs[i + 1]:
                a, b = xs[i - 1], xs[i + 1]
                g = (mp.sqrt(5) - 1) / 2
                c, d = b - g * (b - a), a + g * (b - a)
                hc, hd = sg * f(c), sg * f(d)
                while b - a > mp.mpf(10) ** -18:
                    if hc < hd:
                        b, d, hd = d, c, hc
                        c = b - g * (b - a)
                        hc = sg * f(c)
                    else:
                        a, c, hc = c, d, hd
                        d = a + g * (b - a)
                        hd = sg * f(d)
                x = (a + b) / 2
                out.append((x, f(x), kind))
    return out
