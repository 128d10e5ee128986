"""The yardstick of the 2M + P3 column step with backward-Euler sedimentation (include/cmx.h §24): the Float64 recipe and the property functions are those of
tests/column_implicit_step_cases.py (§21 — the same recurrence); here is what changes because the tendency `a` of §24 is NOT limited — the 2M + P3 tendencies
have no counterpart of the limiter a ≥ −χ/Δt of §19 — and the bounds recounted for that, each a count of roundings from the definition (one rounding = eps/2).
None is fitted to a device run.  Shared by tests/test_mp2m_p3_column_implicit_gpu.py (device results) and tests/test_mp2m_p3_column_implicit_host.py (the
recipe itself on synthetic (a, F, w) of eight species: the yardstick is tested too).

Arrays: a, F, w, out, chi of shape [species, n_col, n_lev] (level 0 the lowest), rho of shape [n_col, n_lev], inv_dz of n_lev values."""
import numpy as np

import column_implicit_step_cases as SC

SHAPES, DTS, EPS = SC.SHAPES, SC.DTS, SC.EPS
recipe, above, explicit = SC.recipe, SC.above, SC.explicit
# the difference between the fall speeds of the velocity entries and the in-kernel w, in eps: taken from column_implicit_step_cases (measured there for the
# SB2006 rain speeds: 2.9 eps, which contains the rounding of g).  The ice speeds are the call's own outputs: no difference at all.
W_ULP = SC.W_ULP

# ---- the identity  out_k (1 + c_k) − out_expl_k = g_k β_{k+1} out_{k+1} -------------------------------------------------------------------------------------
# The count of column_implicit_step_cases up to the point where the limiter is used: the left side is t = fma(G_up, g, h) within (3 + W) eps of |out|(1 + c);
# out_expl = F_up g + h within eps/2 of |a| + g F_k + g F_up; and g (G_{k+1} − F_{k+1}) against g β_{k+1} out_{k+1}, both X1 − X3 + X2 with X1 = A G_{k+2},
# X2 = β r a, X3 = c r F at level k + 1: 7 eps|X1| + 8 eps|X2| + 7 eps|X3|.  There |X2| ≤ F r followed from the limiter.  Here a is free, so X2 stays a term of
# its own: X1 = β out − X2 + X3 and |X3| ≤ F give |X1| ≤ β|out| + |X2| + F, hence 7 eps β|out| + 15 eps|X2| + 14 eps F_{k+1}, all times g_k.  The scale S gains
# g_k β_{k+1} r_{k+1} |a_{k+1}| = g_k|X2|.  Largest coefficient of a term of S: 15 (g|X2|; g F_{k+1} has 14 + 1/2) + 4 (g: inv_dz·rcp(ρ) against the host's
# inv_dz/ρ) + 3 (the host's own Float64 arithmetic) + 3 W (c_k on the left, β_{k+1} and r_{k+1} on the right are formed from the velocity entries' w):
M_IDENTITY = 22.0 + 3.0 * W_ULP


def identity(out, out_expl, a, F, c, beta, g):
    """(|residual|, S) per element: SC.identity with S + g_k β_{k+1} r_{k+1} |a_{k+1}|."""
    res, S = SC.identity(out, out_expl, a, F, c, beta, g)
    return res, S + g * above(beta / (1.0 + c) * np.abs(a))


def surface(G0, F0, beta0, out0, c0, a0):
    """(|residual|, scale) of G_0 = F_0 + β_0 out_0: SC.surface with scale + β_0 r_0 |a_0|.  Both sides are F_0 + X1 − X3 + X2 at level 0 (the count above, without
    the factor g: M_IDENTITY covers it); where X2 = β r a < 0 cancels X1, neither |G_0| nor β_0|out_0| sees it — with the limiter |X2| ≤ F_0 was in the scale."""
    res, sc = SC.surface(G0, F0, beta0, out0)
    return res, sc + beta0 / (1.0 + c0) * np.abs(a0)


# ---- the budget  Σ_k ρ_k out_k/inv_dz_k + G_0 = Σ_k ρ_k a_k/inv_dz_k ----------------------------------------------------------------------------------------
# SC.M_BUDGET counts the 12 roundings between (a, F, w) and (out_k, G_k) and g·ρ Δz = 1 ± 4 eps: 16, per level, relative to what passes through the level.  The
# scale of SC.budget holds the left side only (Σ ρ|out|Δz + |G_0|); with the limiter the right side cannot be larger in magnitude than the mass that is there
# to leave.  Here Σ ρ a Δz is free — a sink a < 0 larger than the content makes out ≈ a with G ≈ 0 — and h = fma(−F, g, a) rounds relative to |a| + g F:
# the scale gains the right side's Σ_k ρ_k|a_k|/inv_dz_k.  The multiple stays.
M_BUDGET = SC.M_BUDGET


def budget(out, G0, a, rho, inv_dz):
    """(|residual|, scale) per species and column: SC.budget with scale + Σ_k ρ_k |a_k|/inv_dz_k."""
    res, sc = SC.budget(out, G0, a, rho, inv_dz)
    mass = (np.maximum(np.asarray(rho, dtype=np.float64), 0.0) / np.asarray(inv_dz, dtype=np.float64)[None, :])[None]
    return res, sc + (mass * np.abs(a)).sum(-1)


# ---- no negativity of its own -------------------------------------------------------------------------------------------------------------------------------
# (1 + c)(χ + Δt out) = χ + Δt a + Δt g G_up (c χ = Δt g F), so with p = χ + Δt a:  χ_k + Δt out_k = r_k (p_k + Δt g_k G_{k+1}) and G_k = w ρ r p + A G_{k+1}.
# A ≥ 0 and p ≥ p⁻ = min(p, 0) give, by induction from the top, G ≥ G⁻ with G⁻_k = A_k G⁻_{k+1} + B⁻_k, B⁻ = w ρ⁺ r p⁻, and
#     χ_k + Δt out_k ≥ L_k = r_k (p⁻_k + Δt g_k G⁻_{k+1}):
# the step leaves nothing below what the tendencies alone (p⁻) and the deficits falling in from above (G⁻ ≤ 0) account for.  L = 0 where p ≥ 0 above and at k.
# Scale: SC.positivity's, χ + Δt|a| + Δt g (F + max_{l>k}(F_l + β_l|a_l|)); |B⁻| ≤ r (F + β|a|) is inside its maximum.
# Multiple: SC.m_positivity without its limiter term is 3 (out) + 4 (g) = 7, + 5·min(levels above, 1 + c_max) for the chain of G (5 roundings per level,
# contracting by A).  On top, the bound itself is formed on the host: 3 eps for its Float64 arithmetic, and from the velocity entries' w where the kernel has
# its own — r_k: W eps of |L|; per level of G⁻: A and r within W eps each and B⁻ = w ρ r p⁻ within 2 W, against |A G⁻_up| + |B⁻| ≤ M: 3 W eps M per level,
# contracting like the chain's own roundings.  Together: 10 + W + (5 + 3 W)·min(levels above, 1 + c_max).


def m_lower(c):
    """The multiple of the lower bound per element, from the Courant numbers c [species, n_col, n_lev]."""
    chain = (SC.m_positivity(c) - 7.0) / 5.0      # min(levels above, 1 + the largest c above)
    return 10.0 + W_ULP + (5.0 + 3.0 * W_ULP) * chain


def lower_bound(chi, a, w, rho, inv_dz, dt):
    """L [species, n_col, n_lev] in Float64: r (p⁻ + Δt g G⁻_up), G⁻ the recurrence of the recipe on B⁻ = w ρ⁺ r p⁻."""
    chi, a, w = (np.asarray(x, dtype=np.float64) for x in (chi, a, w))
    rp = np.maximum(np.asarray(rho, dtype=np.float64), 0.0)[None]
    idz = np.asarray(inv_dz, dtype=np.float64)[None, None, :]
    g = idz / rp
    c = float(dt) * w * idz
    r = 1.0 / (1.0 + c)
    pm = np.minimum(chi + float(dt) * a, 0.0)
    A, Bm = c * r, w * rp * r * pm
    Gm = np.empty_like(Bm)
    n_lev = a.shape[-1]
    Gm[..., n_lev - 1] = Bm[..., n_lev - 1]
    for k in range(n_lev - 2, -1, -1):
        Gm[..., k] = A[..., k] * Gm[..., k + 1] + Bm[..., k]
    return r * (pm + float(dt) * g * above(Gm))


def lower_bound_margin(chi, out, a, F, w, rho, inv_dz, dt):
    """(χ + Δt out − L, scale, m) per element: the assertion is margin ≥ −m·eps·scale."""
    rp = np.maximum(np.asarray(rho, dtype=np.float64), 0.0)[None]
    idz = np.asarray(inv_dz, dtype=np.float64)[None, None, :]
    c, beta, g = dt * w * idz, dt * w * rp, idz / rp
    new, sc = SC.positivity(chi, out, a, F, beta, g, dt)
    return new - lower_bound(chi, a, w, rho, inv_dz, dt), sc, m_lower(c)


def synthetic(seed, n_col, n_lev, dt, n_species=8):
    """SC.synthetic for eight species with an UNLIMITED a: sources and sinks of up to ±3 χ/Δt, so that χ + Δt a < 0 in a good share of the cells."""
    rng = np.random.default_rng(seed)
    shape = (n_species, n_col, n_lev)
    inv_dz = 1.0 / rng.uniform(30.0, 500.0, n_lev)
    rho = rng.uniform(0.3, 1.3, (n_col, n_lev))
    chi = rng.uniform(0.0, 1.0, shape) ** 4 * 1e-3
    w = rng.uniform(0.1, 12.0, shape) * (rng.uniform(size=shape) > 0.1)
    a = rng.normal(0.0, 1e-6, shape) + rng.uniform(-3.0, 1.0, shape) * chi / dt * (rng.uniform(size=shape) < 0.5)
    return dict(inv_dz=inv_dz, rho=rho, chi=chi, w=w, a=a, F=rho[None] * chi * w)
