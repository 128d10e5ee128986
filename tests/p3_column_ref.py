"""Expected result of the 2M + P3 column step (cmx_mp2m_p3_column_tendencies_sedimentation_*) in float64 NumPy, composed from the oracle's
pointwise twins — microphysics_2m_p3_tendencies, p3_terminal_velocities, sb2006_warm_rain_tendencies (vt_rai_n, vt_rai_m),
sb2006_cloud_terminal_velocity — plus the host model's first-order upwind flux divergence, restated here as in include/cmx.h:

    F_k = ρ_k χ_k w_k,   ∂χ_k/∂t += (F_{k+1} − F_k)·inv_dz[k]/ρ_k,   F_{n_lev} = 0     (level 0 lowest; ρ, χ clamped at 0)

log λ is an ARGUMENT: the GPU tests pass the device's own log_lambda output (non-finite values replaced by 0), so that the comparison
measures the entry and not two Brent solvers' iterates; `check_log_lambda` compares the device's log λ with the oracle's shape solve
separately, at a converged budget.  The flux step is the host model's scheme, not the reference's ("parity unpinned").

Also the mixed-phase state generator of tests/test_mp2m_p3_gpu.py, restated and laid out as columns."""
import numpy as np

from cmx import _abi
from cmx import parameters as P

import parity

NAMES = ("dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt", "dq_ice_dt", "dn_ice_dt", "dq_rim_dt", "db_rim_dt")
IN_NAMES = ("rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai", "q_ice", "n_ice", "q_rim", "b_rim")
NP = {"f32": np.float32, "f64": np.float64}
MAX_FLIPPED = 1e-3        # fraction of points allowed on another Brent path / root (tests/test_p3_gpu.py)


def states(n_col, n_lev, seed=11, f32_safe=False):
    """Mixed-phase states as (n_col, n_lev) float64 columns (the generator of tests/test_mp2m_p3_gpu.py::_states).  `f32_safe`: keep L_ice
    and B_rim out of the blending band of the reference's regularised ratios (F_rim = L_rim/L_ice, ρ_rim = L_rim/B_rim are blended to 0 for
    denominators in (eps/4, 42 eps), Utilities.jl:445-488).  In Float32 that band is 3e-8…5e-6 — where every realistic rime volume lies —
    and the blending weight (1 − a)^(…) with a ≈ 1e-7 is not computable in Float32 arithmetic, the reference's included; Float32 parity is
    therefore checked on unrimed states and on states with B_rim above the band."""
    n = n_col * n_lev
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.4, 1.3, n)
    T = rng.uniform(215.0, 295.0, n)
    q_lcl = np.where(rng.random(n) < 0.7, 10 ** rng.uniform(-6, -3, n), 0.0)
    q_rai = np.where(rng.random(n) < 0.6, 10 ** rng.uniform(-7, -3, n), 0.0)
    n_lcl = 10 ** rng.uniform(6, 9, n)
    n_rai = 10 ** rng.uniform(1, 6, n)
    q_ice = np.where(rng.random(n) < 0.8, 10 ** rng.uniform(-7, -3, n), 0.0)
    n_ice = 10 ** rng.uniform(2, 6, n)
    F = np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0.05, 0.9, n))
    q_rim = F * q_ice
    b_rim = q_rim / rng.uniform(200, 800, n)
    if f32_safe:
        q_ice = np.where(rng.random(n) < 0.8, 10 ** rng.uniform(-4.5, -2.5, n), 0.0)
        heavy = (rng.random(n) < 0.4) & (q_ice > 0)
        q_ice = np.where(heavy, rng.uniform(1.5e-2, 3e-2, n), q_ice)
        q_rim = np.where(heavy, rng.uniform(0.5, 0.9, n) * q_ice, 0.0)
        b_rim = np.where(heavy, q_rim / rng.uniform(200, 400, n), 0.0)
    q_tot = q_lcl + q_rai + q_ice + 10 ** rng.uniform(-5, -2, n)
    neg = rng.random(n) < 0.01                       # a few slightly negative inputs: the clamps of BMT:912-921
    q_rai = np.where(neg, -1e-9, q_rai)
    s = dict(rho=rho, T=T, q_tot=q_tot, q_lcl=q_lcl, n_lcl=n_lcl, q_rai=q_rai, n_rai=n_rai, q_ice=q_ice, n_ice=n_ice, q_rim=q_rim, b_rim=b_rim)
    return {k: v.reshape(n_col, n_lev) for k, v in s.items()}


def inv_dz(n_lev, seed=0):
    """1/Δz_k for layers of 30…500 m (float64)."""
    return 1.0 / (30.0 + 470.0 * np.random.default_rng(seed).random(n_lev))


def as_ft(cols, ft):
    """The columns rounded to the device's float type, as float64 (what the oracle must see)."""
    return {k: np.asarray(v).astype(NP[ft]).astype(np.float64) for k, v in cols.items()}


def products(cols, ft):
    """(ρ q_ice, ρ n_ice, ρ q_rim, ρ b_rim), each ONE product rounded in the device's float type — the operands of step 1 — as float64."""
    r = np.asarray(cols["rho"]).astype(NP[ft])
    return [(r * np.asarray(cols[k]).astype(NP[ft])).astype(np.float64) for k in ("q_ice", "n_ice", "q_rim", "b_rim")]


def upwind(F):
    """The flux entering each cell through its upper face: the flux leaving the cell above, 0 at the model top."""
    return np.concatenate([F[:, 1:], np.zeros_like(F[:, :1])], axis=1)


def expected(oracle, ft, cols, dz, log_lambda, *, limited=True, vel="sb", cloud=False, shift=None, p=1e-6, aspect=True, nthreads=8):
    """cols: the 11 state columns (n_col, n_lev) AS THE DEVICE HOLDS THEM (rounded to ft); dz: inv_dz (n_lev) likewise; log_lambda: the
    device's output with non-finite values replaced by 0.  Float64 arithmetic with ft's gates.
    → dict(tend[8], scale[8] (the oracle's Σ|terms| widened by (F_up + F)·inv_dz/ρ of the species), v_ice_n, v_ice_m, precip_rai, precip_ice)."""
    c = {k: np.asarray(cols[k], dtype=np.float64) for k in IN_NAMES}
    shape = c["rho"].shape
    flat = [c[k].reshape(-1) for k in IN_NAMES]
    gates = ft == "f32"
    mp = P.Microphysics2MParams("f64", with_ice=True, is_limited=limited)
    tps = P.ThermodynamicsParameters("f64")
    flags = mp.ice.flags | (0 if aspect else _abi.CMX_P3_NO_ASPECT_RATIO)
    ll = np.asarray(log_lambda, dtype=np.float64).reshape(-1)
    sh = None if shift is None else np.asarray(shift, dtype=np.float64).reshape(-1)
    tend, scale = oracle.microphysics_2m_p3_tendencies(_abi.F64, mp.warm_rain.c, mp.ice.c, tps, flags, *flat, ll, sh, float32_gates=gates, nthreads=nthreads)
    tend, scale = tend.astype(np.float64).reshape(8, *shape), scale.astype(np.float64).reshape(8, *shape)
    rq, rn, x3, x4 = [a.reshape(-1) for a in products(cols, ft)]
    v_n, v_m = oracle.p3_terminal_velocities(_abi.F64, mp.ice.c.scheme, mp.ice.c.vel_ice, mp.ice.c.quad, flags & ~_abi.CMX_P3_RAIN_PDF_LIMITED, rq, rn, x3, x4,
                                             flat[0], ll, p=p, float32_gates=gates, nthreads=nthreads)
    v_n, v_m = v_n.reshape(shape), v_m.reshape(shape)
    wflags = (_abi.CMX_SB2006_LIMITED if limited else 0) | (_abi.CMX_VEL_SB2006 if vel == "sb" else _abi.CMX_VEL_CHEN2022)
    warm = oracle.sb2006_warm_rain_tendencies(_abi.F64, mp.warm_rain.c, tps, P.rain_vel_params("f64"), wflags, *flat[:7], float32_gates=gates,
                                              nthreads=nthreads, want_scale=False)
    w_n, w_m = warm["vt_rai_n"].reshape(shape), warm["vt_rai_m"].reshape(shape)
    cl = {k: np.maximum(c[k], 0.0) for k in IN_NAMES}       # clamp_to_nonneg
    rho = cl["rho"]
    speeds = {"dq_rai_dt": ("q_rai", w_m), "dn_rai_dt": ("n_rai", w_n), "dq_ice_dt": ("q_ice", v_m), "dn_ice_dt": ("n_ice", v_n),
              "dq_rim_dt": ("q_rim", v_m), "db_rim_dt": ("b_rim", v_m)}
    if cloud:
        c_n, c_m = oracle.sb2006_cloud_terminal_velocity(_abi.F64, mp.warm_rain.c.seifert_beheng.pdf_c, P.StokesRegimeVelType("f64"), cl["q_lcl"].reshape(-1),
                                                         rho.reshape(-1), (rho * cl["n_lcl"]).reshape(-1), float32_gates=gates)
        speeds["dq_lcl_dt"] = ("q_lcl", c_m.reshape(shape))
        speeds["dn_lcl_dt"] = ("n_lcl", c_n.reshape(shape))
    g = np.asarray(dz, dtype=np.float64)[None, :] / rho
    out = {"tend": tend, "scale": scale, "v_ice_n": v_n, "v_ice_m": v_m}
    for q, name in enumerate(NAMES):
        if name not in speeds:
            continue
        chi, w = speeds[name]
        F = (rho * cl[chi]) * w
        up = upwind(F)
        tend[q] = tend[q] + (up - F) * g
        scale[q] = scale[q] + (up + F) * g
        if name == "dq_rai_dt":
            out["precip_rai"] = F[:, 0].copy()
        if name == "dq_ice_dt":
            out["precip_ice"] = F[:, 0].copy()
    return out


def assert_tendencies(got, exp, ft, what=""):
    """The metric of tests/test_mp2m_p3_gpu.py on all eight columns, every point: |x − ref| ≤ RTOL·|ref| + CTOL·scale.  `got`: name → array."""
    worst = {}
    for q, name in enumerate(NAMES):
        x = np.asarray(got[name], dtype=np.float64)
        ref, scale = exp["tend"][q], exp["scale"][q]
        assert x.shape == ref.shape and np.all(np.isfinite(x)), (what, name)
        tol = parity.RTOL[ft] * np.abs(ref) + parity.CTOL[ft] * scale
        err = np.abs(x - ref) / np.maximum(tol, 1e-300)
        err[(x == 0) & (ref == 0)] = 0
        worst[name] = float(err.max())
        j = np.unravel_index(int(np.argmax(err)), err.shape)
        print(f"[2M+P3 column] {what} {name}: worst err/tol {worst[name]:.3f} at {j}")
    for name, w in worst.items():
        assert w <= 1.0, (what, name, w)
    return worst


def assert_ice_speeds(got_n, got_m, exp, ft, what=""):
    """The bound of tests/test_p3_gpu.py::test_random_state_fall_speed_parity: the same zero pattern, relative error ≤ RTOL at the same log λ."""
    rep = {}
    for name, x, r in (("v_ice_n", got_n, exp["v_ice_n"]), ("v_ice_m", got_m, exp["v_ice_m"])):
        x, r = np.asarray(x, dtype=np.float64), np.asarray(r, dtype=np.float64)
        assert np.array_equal(x == 0, r == 0), (what, name)
        nz = r != 0
        rep[name] = float((np.abs(x[nz] - r[nz]) / np.abs(r[nz])).max(initial=0.0))
        print(f"[2M+P3 column] {what} {name}: worst relative error {rep[name]:.3e}")
    for name, e in rep.items():
        assert e <= parity.RTOL[ft], (what, name, e)
    return rep


def check_log_lambda(oracle, ft, log_lambda, cols, *, slope_flags=0, what=""):
    """The device's log λ (solved at brent_iters = 40) against oracle.p3_shape at the same converged budget on the same products, with the
    bound of tests/test_p3_gpu.py::_solver_parity: the same −Inf pattern, finite values inside [2, 17], relative error ≤ RTOL except for at
    most MAX_FLIPPED of the points (another Brent path / root of the multi-rooted residual)."""
    ll = np.asarray(log_lambda, dtype=np.float64).reshape(-1)
    rq, rn, x3, x4 = [a.reshape(-1) for a in products(cols, ft)]
    p64 = P.ParametersP3("f64", "constant" if slope_flags else "powerlaw").c
    ref = oracle.p3_shape(_abi.F64, p64, slope_flags, rq, rn, x3, x4, float32_gates=(ft == "f32"), maxiters=40, nthreads=8)["log_lambda"]
    assert np.array_equal(np.isneginf(ll), np.isneginf(ref)), what
    fin = np.isfinite(ref)
    assert np.all(np.isfinite(ll[fin])) and np.all((ll[fin] >= 2) & (ll[fin] <= 17)), what
    err = np.zeros_like(ref)
    err[fin] = np.abs(ll[fin] - ref[fin]) / np.abs(ref[fin])
    flipped = fin & (err > parity.RTOL[ft])
    print(f"[2M+P3 column] {what} log λ: {int(fin.sum())} states with ice, {int(flipped.sum())} flipped, worst of the rest {err[fin & ~flipped].max(initial=0.0):.3e}")
    assert flipped.sum() <= MAX_FLIPPED * fin.sum(), (what, int(flipped.sum()), int(fin.sum()))
    return int(fin.sum()), int((~fin).sum())
