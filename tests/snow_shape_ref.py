"""Float64 NumPy restatement of the Chen-2022 snow fall speed with and without a snow shape — the reference for tests/test_snow_shape_*.py.

    CM1.terminal_velocity(snow, Ch2022.large_ice, ρ, q)          src/Microphysics1M.jl:272-297   (fixed aspect ratio ϕ^κ)
    CM1.terminal_velocity(snow, Ch2022.large_ice, ρ, q, shape)   src/Microphysics1M.jl:299-324   (ϕ_av^κ, CM1.aspect_ratio_coeffs :155-195)
    CM1.lambda_inverse / get_n0                                  src/Microphysics1M.jl:83-86, 126-152
    CO.Chen2022_vel_coeffs(large ice), Chen2022_exponential_pdf  src/Common.jl:327-350, 414-422

Written from the reference's formulas, independent of csrc/ (no log2-domain folding).  It is pinned by tests/test_snow_shape_host.py: the B4 large-ice
coefficients of test/common_functions_tests.jl:166-180 (tests/golden/snow_shape_kats.json), the unshaped known answer of
test/microphysics1M_tests.jl:77 (tests/golden/mp1m_kats.json), the oracle's unshaped snow speed and the reference's qualitative shape checks."""
from __future__ import annotations

import math

import numpy as np

EPS_NUMERICS = {"f32": float(np.cbrt(np.float64(np.finfo(np.float32).tiny))), "f64": float(np.cbrt(np.finfo(np.float64).tiny))}


class Oblate:
    pass


class Prolate:
    pass


def large_ice_coeffs(large, rho_a, rho_i):
    """CO.Chen2022_vel_coeffs(::Chen2022VelTypeLargeIce, ρₐ, ρᵢ) → (aiu, bi, ciu), each a pair; ρₐ may be an array."""
    A, B, Cc, E, F, G, H = ([float(x) for x in getattr(large, k)] for k in "ABCEFGH")
    rho_a = np.maximum(np.asarray(rho_a, dtype=np.float64), 0.0)
    l, sq = math.log(rho_i), math.sqrt(rho_i)
    Al = A[0] + A[1] * l + A[2] / (rho_i * sq)
    Bl = math.exp(B[0] + B[1] * l ** 2 + B[2] * l)
    Cl = math.exp(Cc[0] + Cc[1] / l + Cc[2] / rho_i)
    El = E[0] + E[1] * l * sq + E[2] * sq
    Fl = F[0] + F[1] * l - math.exp(math.log(-F[2]) - rho_i)
    Gl = 1 / (G[0] + G[1] * l * sq + G[2] / sq)
    Hl = H[0] + H[1] * rho_i ** 2 * sq + math.exp(math.log(-H[2]) - rho_i)
    with np.errstate(divide="ignore"):
        ai = (Bl * rho_a ** Al, El * rho_a ** Al * np.exp(Hl * rho_a))
    bi = (Cl, Fl)
    ci = (0.0, Gl)
    return tuple(a * 1000.0 ** b for a, b in zip(ai, bi)), bi, tuple(c * 1000.0 for c in ci)


def lambda_inverse_snow(snow, q, rho, eps):
    """CM1.lambda_inverse(snow.pdf, snow.mass, q, ρ): the radius slope parameter, floored at r0·1e-5."""
    m = snow.mass
    q, rho = np.asarray(q, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n0 = np.where(q > eps, snow.mu * (rho * np.maximum(q, eps)) ** snow.nu, 0.0)
        mexp = m.me + m.delta_m
        denom = m.chi_m * m.m0 * np.maximum(n0, eps) * m.gamma_coeff
        lam = (np.maximum(rho, 0.0) * np.maximum(q, 0.0) * m.r0 ** mexp / denom) ** (1 / (mexp + 1))
    return np.maximum(m.r0 * 1e-5, lam)


def aspect_ratio_coeffs(shape, snow):
    """CM1.aspect_ratio_coeffs(shape, snow.mass, snow.area, snow.ρᵢ) → (ϕ₀, α, κ)."""
    m, a, ri = snow.mass, snow.area, snow.rho_i
    mexp, aexp = m.me + m.delta_m, a.ae + a.delta_a
    if isinstance(shape, Oblate):
        alpha = mexp - 3 / 2 * aexp
        return 3 * math.sqrt(math.pi) / 4 / ri * m.chi_m * m.m0 / (a.chi_a * a.a0) ** 1.5 / (2 * m.r0) ** alpha, alpha, 1 / 3
    alpha = 3 * aexp - 2 * mexp
    return 16 * ri ** 2 / 9 / math.pi * (a.chi_a * a.a0) ** 3 / (m.chi_m * m.m0) ** 2 / (2 * m.r0) ** alpha, alpha, -1 / 6


def exponential_pdf(a, b, c, lam_inv, k=3):
    """CO.Chen2022_exponential_pdf(a, b, c, λ⁻¹, k)."""
    d = k + 1
    return a * np.exp(-d * np.log(lam_inv) - (b + d) * np.log(1 / lam_inv + c)) * math.gamma(b + d) / math.factorial(k)


def snow_velocity(mp, chen_ice, rho, q, shape=None, ft="f64"):
    """w_sno over arrays (float64): `mp` = Microphysics1MParams(...).c, `chen_ice` = Chen2022VelTypeIce(...); shape None / Oblate() / Prolate().
    ft selects ϵ_numerics (the gates of the float type)."""
    snow = mp.snow
    eps = EPS_NUMERICS[ft]
    rho, q = np.asarray(rho, dtype=np.float64), np.asarray(q, dtype=np.float64)
    aiu, bi, ciu = large_ice_coeffs(chen_ice.large_ice, rho, float(snow.rho_i))
    lr = lambda_inverse_snow(snow, q, rho, eps)
    ld = 2 * lr
    if shape is None:
        f = float(snow.phi) ** float(snow.kappa)
    else:
        phi0, alpha, kappa = aspect_ratio_coeffs(shape, snow)
        gam = snow.gamma_aspect_oblate if isinstance(shape, Oblate) else snow.gamma_aspect_prolate
        f = (phi0 * lr ** alpha * gam) ** kappa
    with np.errstate(invalid="ignore", over="ignore"):
        w = f * exponential_pdf(aiu[0], bi[0], ciu[0], ld) + f * exponential_pdf(aiu[1], bi[1], ciu[1], ld)
    w = np.maximum(0.0, w)
    return np.where(q > eps, w, 0.0)
