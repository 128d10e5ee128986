"""Float64 NumPy restatement of the SB2006 precipitation susceptibilities (src/PrecipitationSusceptibility.jl:36-79): the logarithmic derivatives of
dq_rai_dt of CM2.autoconversion (src/Microphysics2M.jl:396-427) and CM2.accretion (:445-470) with respect to ln|q_lcl|, ln|q_rai|, ln|N_lcl|, written
as the closed forms of include/cmx.h §(12) — in the arrangement of that header (u, G, h), which is NOT the device's (one division, none by 1 − τ^a).

`eps` is a parameter: the gates of the reference depend on the float type (ϵ_numerics_2M_* = eps(FT), src/Utilities.jl:325,332), so a Float32 result is
compared with this float64 arithmetic at the Float32 gates.  `acnv` / `accr` are anything with the fields of cmx_acnv_sb2006 / cmx_accr_sb2006.

NaN contract (cmx's own, include/cmx.h): a process whose gate fires (its dq_rai_dt is zeroed) has NaN in all three outputs, and so has a point with a
NaN input or ρ = 0.  Test infrastructure only."""
import numpy as np

EPS = {"f32": float(np.finfo(np.float32).eps), "f64": float(np.finfo(np.float64).eps)}
FIELDS = ("d_ln_q_lcl", "d_ln_q_rai", "d_ln_N_lcl")


def _abs_inputs(q_lcl, q_rai, rho, N_lcl):
    a = [np.abs(np.asarray(x, dtype=np.float64)) for x in (q_lcl, q_rai, rho, N_lcl)]
    a = np.broadcast_arrays(*a)
    bad = np.isnan(a[0]) | np.isnan(a[1]) | np.isnan(a[2]) | np.isnan(a[3]) | (a[2] == 0)
    return a, bad


def taus(q_lcl, q_rai):
    """(τ, 1 − τ) as the quotients q_rai/(q_lcl + q_rai), q_lcl/(q_lcl + q_rai)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return q_rai / (q_lcl + q_rai), q_lcl / (q_lcl + q_rai)


def x_ratio(acnv, q_lcl, rho, N_lcl):
    """x̄_c/x_star of the absolute inputs"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(rho) * np.abs(q_lcl) / np.abs(N_lcl) / float(acnv.x_star)


def autoconversion(acnv, q_lcl, q_rai, rho, N_lcl, eps):
    (ql, qr, rh, N), bad = _abs_inputs(q_lcl, q_rai, rho, N_lcl)
    A, a, b = float(acnv.A), float(acnv.a), float(acnv.b)
    tau, omt = taus(ql, qr)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ta = tau ** a
        u = A * ta * (1 - ta) ** b / omt ** 2
        G = u / (1 + u) * (a - a * b * ta / (1 - ta) + 2 * tau / omt)
        G = np.where(qr < eps, 0.0, G)                                     # the ifelse of CM2 :411
        S_r = omt * G
        clipped = ~(rh * ql / N < float(acnv.x_star))                      # the min of CM2 :406
    gate = bad | (ql < eps) | (N < eps)                                    # CM2 :420
    nan = lambda v: np.where(gate, np.nan, v)  # noqa: E731
    return {"d_ln_q_lcl": nan(np.where(clipped, 2.0, 4.0) - S_r), "d_ln_q_rai": nan(S_r), "d_ln_N_lcl": nan(np.where(clipped, 0.0, -2.0))}


def accretion(accr, q_lcl, q_rai, rho, N_lcl, eps):
    (ql, qr, rh, N), bad = _abs_inputs(q_lcl, q_rai, rho, N_lcl)
    tau, omt = taus(ql, qr)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = omt * float(accr.c) * float(accr.tau_0) / (tau + float(accr.tau_0))
    gate = bad | (ql < eps) | (qr < eps) | (N < eps)                       # CM2 :463
    nan = lambda v: np.where(gate, np.nan, v)  # noqa: E731
    return {"d_ln_q_lcl": nan(1 - h), "d_ln_q_rai": nan(1 + h), "d_ln_N_lcl": nan(np.zeros_like(h))}


# ---- the reference test's own arrangement (test/precipitation_susceptibility_tests.jl:11-29) ---------------------------------------------

def d_ln_phi_au_d_ln_tau(acnv, tau):
    A, a, b = float(acnv.A), float(acnv.a), float(acnv.b)
    return -(A * tau ** a * (1 - tau ** a) ** (b - 1) * (a * (tau - 1) * ((b + 1) * tau ** a - 1) - 2 * tau * (tau ** a - 1))) / (
        A * (tau - 1) * tau ** a * (1 - tau ** a) ** b + (tau - 1) ** 3)


def d_ln_phi_acc_d_ln_tau(accr, tau):
    return float(accr.c) * float(accr.tau_0) / (tau + float(accr.tau_0))


# ---- the random draw of the parity tests (tests/test_precip_susceptibility_*.py) -----------------------------------------------------------

def random_states(n, seed=1234):
    """q_lcl, q_rai ~ log-U[1e-9, 5e-3] with 2 % exact zeros and 1 % slightly negative values (−log-U[1e-9, 1e-6]: they enter through abs),
    ρ ~ U[0.3, 1.3], N_lcl ~ log-U[1e6, 3e9] with 1 % zeros.  The tests assert that every branch of the closed forms is populated."""
    g = np.random.default_rng(seed)

    def lu(lo, hi):
        return np.exp(g.uniform(np.log(lo), np.log(hi), n))

    def content():
        q = lu(1e-9, 5e-3)
        small = lu(1e-9, 1e-6)
        r = g.random(n)
        q[r < 0.02] = 0.0
        neg = (r >= 0.02) & (r < 0.03)
        q[neg] = -small[neg]
        return q
    q_lcl, q_rai = content(), content()
    rho = g.uniform(0.3, 1.3, n)
    N_lcl = lu(1e6, 3e9)
    N_lcl[g.random(n) < 0.01] = 0.0
    return q_lcl, q_rai, rho, N_lcl


def near_clip(acnv, q_lcl, rho, N_lcl, margin=1e-5):
    """|x̄_c/x_star − 1| < margin: a rounding may pick the other branch of the min of CM2 :406"""
    with np.errstate(invalid="ignore"):
        return np.abs(x_ratio(acnv, q_lcl, rho, N_lcl) - 1) < margin
