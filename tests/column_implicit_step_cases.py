"""The Float64 host recipe of the column steps with backward-Euler sedimentation (include/cmx.h §21) and the three properties the device tests assert of
the entries — the defining identity against the explicit step, the column budget, positivity — as NumPy code shared by
tests/test_column_implicit_step_gpu.py (which applies the property functions to the device results) and tests/test_column_implicit_step_host.py (which
applies them to the recipe itself on synthetic (a, F, w): the yardstick is tested too).

Arrays: a, F, w, out of shape [4, n_col, n_lev] (species, column, level; level 0 the lowest), rho of shape [n_col, n_lev], inv_dz of n_lev values."""
import numpy as np

# around the kernel's chunk of 256 points and the column top; (2, 600): a column over three chunks, the carry crosses two chunk boundaries
SHAPES = [(1, 1), (7, 1), (2, 2), (4, 64), (3, 85), (65, 63), (1, 255), (1, 256), (1, 257), (2, 600)]
DTS = (1.0, 30.0, 300.0)
EPS = {"f32": 2.0 ** -23, "f64": 2.0 ** -52}

# ---- the multiples of eps(FT), counted from the definition (one rounding = eps/2) -----------------------------------------------------------------------
# W_ULP: the measured difference between the fall speeds of the velocity entries and the in-kernel w, in eps (see test_the_defining_identity…): an upper
# bound — 2.9 eps (SB2006), 1.8 eps (1-moment) in a Float64 device run, which contains the rounding of g = inv_dz·rsqrt(ρ)² resp. inv_dz·rcp(ρ) as well
W_ULP = 3.0
# The identity  out_k (1 + c_k) − out_expl_k = g_k β_{k+1} out_{k+1}.  Device side: out = t·r with t = fma(G_up, g, h), h = fma(−F, g, a) — h has the bits of the
# explicit entry's inner fma and cancels; t, the product, r = 1/D, D = 1 + c, c = τ·inv_dz, τ = Δt·w: out (1 + c) = t within (6 roundings + w) = (3 + W) eps of
# |out|(1 + c); out_expl = F_up g + h within eps/2 of |a| + g F_k + g F_up.  Then g (G_{k+1} − F_{k+1}) against g β_{k+1} out_{k+1}: both are
# X1 − X3 + X2 with X1 = A G_{k+2}, X2 = β r a, X3 = c r F at level k + 1.  In G (fma, A = c·r, B = fma(β, a, F)·r, β = τ ρ) X1 carries 8 roundings, X2 9,
# F r − F = −X3 7; in β out (t, h, the product, r) 6, 7 and 7: 7 eps|X1| + 8 eps|X2| + 7 eps|X3|, + 3 W.  With the limiter a ≥ −χ/Δt, so |X2| ≤ F r where
# a < 0, and A + r = 1: |X1| ≤ β|out| + F, hence ≤ 8 eps β|out| + 15 eps F_{k+1}.  g itself (inv_dz·rsqrt², inv_dz·rcp: ≤ 4 eps against the host's inv_dz/ρ)
# multiplies the right side.  The host's own Float64 arithmetic (≈ 6 roundings of terms of S) matters for FT = Float64 only: 3 eps.
# Largest coefficient of a term of S: 15 + 1/2 (g F_{k+1}) + 4 (g) + 3 (host) + 3 W, rounded up:
M_IDENTITY = 24.0 + 3.0 * W_ULP
# The budget: every level is consistent with the G above and below it to the roundings between (a, F, w) and (out_k, G_k) — τ, c, β, D, r, A, the fma and the
# product of B, the fma of G, h, t, the product of out: 12 — and to g·ρ Δz = 1 ± 4 eps: 16.  G_k enters level k and level k − 1 with the same bits, so the errors of
# G itself cancel in the sum.  (Not a worst-case bound: a level's inconsistency is relative to its throughput β|out| = c ρ Δz|out|, which at c ≫ 1 the scale
# the budget is measured in contains through G_0, where the throughput ends up, and not level by level.)
M_BUDGET = 16.0


def m_positivity(c):
    """The multiple of the positivity bound per element, from the Courant numbers c [4, n_col, n_lev]: out = (G_up g + h) r within 3 eps of
    |out| ≤ r(|a| + g F + g M), M = max over the levels above of F + β|a| ≥ G; g within 4 eps; Δt·a ≥ −χ(1 + 3/2 eps): 7.  The rounding of G compounds down
    the chain: E_k ≤ A_k E_{k+1} + 5 eps M (the fma, A, and in B the fma, the product and r; c, τ, β once more, each relative to A G_up + |B| ≤ M).  One term
    per level above, and the terms contract by A = c/(1 + c) ≤ c_max/(1 + c_max) per level, so their sum is at most 1 + c_max of them, c_max the largest c of
    that species in the levels above k: the multiple is 7 + 5·min(n_lev − 1 − k, 1 + c_max)."""
    n_lev = c.shape[-1]
    above_max = np.zeros_like(c)
    for k in range(n_lev - 2, -1, -1):
        above_max[..., k] = np.maximum(above_max[..., k + 1], c[..., k + 1])
    n_above = n_lev - 1 - np.arange(n_lev, dtype=np.float64)
    return 7.0 + 5.0 * np.minimum(n_above, 1.0 + above_max)


def recipe(a, F, w, rho, inv_dz, dt):
    """(out, G, c, beta, g) of the definition of §21 in Float64, G[..., 0] the surface flux."""
    a, F, w = (np.asarray(x, dtype=np.float64) for x in (a, F, w))
    rp = np.maximum(np.asarray(rho, dtype=np.float64), 0.0)[None]
    idz = np.asarray(inv_dz, dtype=np.float64)[None, None, :]
    g = idz / rp
    tau = float(dt) * w
    c, beta = tau * idz, tau * rp
    r = 1.0 / (1.0 + c)
    A, B = c * r, (beta * a + F) * r
    G = np.empty_like(B)
    n_lev = a.shape[-1]
    G[..., n_lev - 1] = B[..., n_lev - 1]
    for k in range(n_lev - 2, -1, -1):
        G[..., k] = A[..., k] * G[..., k + 1] + B[..., k]
    out = (above(G) * g - F * g + a) * r
    return out, G, c, beta, g


def above(x):
    """x at level k + 1, 0 at the column top."""
    up = np.zeros_like(x)
    up[..., :-1] = x[..., 1:]
    return up


def explicit(a, F, rho, inv_dz):
    """The explicit combination of §20 in Float64."""
    g = np.asarray(inv_dz, dtype=np.float64)[None, None, :] / np.maximum(np.asarray(rho, dtype=np.float64), 0.0)[None]
    return above(F) * g - F * g + a


def identity(out, out_expl, a, F, c, beta, g):
    """(|residual|, S) per element of  out_k (1 + c_k) − out_expl_k = g_k β_{k+1} out_{k+1}  (top: right side 0); S the sum of the magnitudes of the terms."""
    rhs = g * above(beta * out)
    res = np.abs(out * (1.0 + c) - out_expl - rhs)
    S = np.abs(out) * (1.0 + c) + np.abs(a) + g * np.abs(F) + g * above(np.abs(F)) + g * above(beta * np.abs(out))
    return res, S


def surface(G0, F0, beta0, out0):
    """(|residual|, scale) of G_0 = F_0 + β_0 out_0."""
    return np.abs(G0 - F0 - beta0 * out0), np.abs(G0) + np.abs(F0) + beta0 * np.abs(out0)


def budget(out, G0, a, rho, inv_dz):
    """(|residual|, scale) per species and column of  Σ_k ρ_k out_k/inv_dz_k + G_0 = Σ_k ρ_k a_k/inv_dz_k."""
    mass = (np.maximum(np.asarray(rho, dtype=np.float64), 0.0) / np.asarray(inv_dz, dtype=np.float64)[None, :])[None]
    res = np.abs((mass * out).sum(-1) + G0 - (mass * a).sum(-1))
    return res, (mass * np.abs(out)).sum(-1) + np.abs(G0)


def positivity(chi, out, a, F, beta, g, dt):
    """(χ + Δt out, scale) per element; scale = χ + Δt|a| + Δt g (F_k + max_{l>k}(F_l + β_l|a_l|)): rounding in G is relative to the content of the cells above."""
    M = F + beta * np.abs(a)
    run = np.zeros_like(M)
    for k in range(M.shape[-1] - 2, -1, -1):
        run[..., k] = np.maximum(run[..., k + 1], M[..., k + 1])
    return chi + dt * out, chi + dt * np.abs(a) + dt * g * (F + run)


def synthetic(seed, n_col, n_lev, dt):
    """Random columns in the regime the step exists for: Δz ∈ [30, 500] m, w ∈ [0.1, 9] m/s (some cells at rest), χ ≥ 0, a ≥ −χ/Δt."""
    rng = np.random.default_rng(seed)
    inv_dz = 1.0 / rng.uniform(30.0, 500.0, n_lev)
    rho = rng.uniform(0.3, 1.3, (n_col, n_lev))
    chi = rng.uniform(0.0, 1.0, (4, n_col, n_lev)) ** 4 * 1e-3
    w = rng.uniform(0.1, 9.0, (4, n_col, n_lev)) * (rng.uniform(size=(4, n_col, n_lev)) > 0.1)
    a = np.maximum(rng.normal(0.0, 1e-6, (4, n_col, n_lev)), -chi / dt)
    return dict(inv_dz=inv_dz, rho=rho, chi=chi, w=w, a=a, F=rho[None] * chi * w)
