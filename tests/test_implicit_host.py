"""The linearly implicit tendency r = (I − Δt J)⁻¹ f (include/cmx.h §18) without a GPU: the driver's implicit_point (csrc/cmx_jacobian.hpp) in the host build
tests/native/implicit_host.cpp — on a linear toy scheme f = M s, where the solve alone can be compared with a closed form, and on the two real schemes against
the host build of their Jacobian (tests/native/derivatives_host.cpp) — and the argument statuses of the device entries.  tests/implicit_cases.py has the
states and the measures.

Worst values of the host build over the sets of implicit_cases (Δt = 1, 30, 300 s), the fused solve | LAPACK in the same precision:
  backward error ω    SB2006 Float32 1.2e-7 | 8.2e-8   Float64 6.2e-16 | 1.5e-9      1-moment Float32 1.1e-7 | 8.1e-8   Float64 4.3e-16 | 3.2e-12
  (numpy.linalg.solve computes in Float64 and rounds the result, so in Float32 the bound in effect is its floor, 16 eps = 1.9e-6; without the driver's
  refinement step the fused solve stood at 2.3e-4 / 3.5e-13)
  forward error / (κ∞ eps), Float64   SB2006 2.7 (no point left out for κ∞ > 1e6, largest κ∞ 8.0e5)   1-moment 2.0 (at most 0.10 % left out, Δt = 300 s)
No Δt had to be dropped from the forward check."""
import ctypes as C

import numpy as np
import pytest

import implicit_cases as IC
import jacobian_1m_cases as J1
import jacobian_cases as JC
import jacobian_host_build as JH
from jacobian_host_build import NPT, _same_bits, host_fixture
from cmx import _abi, _lib
from cmx import parameters as P

host = host_fixture("implicit_host")
derivatives = host_fixture("derivatives_host")
FTS = ["f64", "f32"]


# ---- the toy scheme: f = M s ------------------------------------------------------------------------------------------------------------------------
def toy(host, ft, M, s, dt, k=0, rho=None):
    n = np.asarray(s[0]).size
    cols = [np.ones(n) if rho is None else rho] + list(s)
    return IC.host_implicit(host, "toy", ft, IC.head_toy(ft, M), dt, cols, k=k)


def closed_form(ft, M, s, dt):
    """(I − Δt M)⁻¹ M s in Float64 from M and s as the float type holds them."""
    M64 = np.asarray(M, dtype=NPT[ft]).astype(np.float64)
    s64 = np.stack([np.asarray(c, dtype=NPT[ft]).astype(np.float64) for c in s], axis=1)
    A = np.eye(4) - float(NPT[ft](dt)) * M64
    return np.linalg.solve(A[None], (s64 @ M64.T)[..., None])[..., 0], A


# entries from 4e-10 to 8e+10 once the units are applied: a sink on the diagonal, every species feeds every other (f = M s without cancellation: all terms of a
# row have one sign), the units of species 1 and 3 are 2^33 ≈ 8.6e9 and 2^17 times those of species 0 and 2 — SB2006's kg⁻¹ against kg kg⁻¹
G = -np.array([[4.0, 0.5, 0.25, 1.0], [0.75, 3.0, 0.5, 0.125], [1.0, 0.25, 5.0, 0.5], [0.5, 1.0, 0.75, 2.0]]) / 64.0
UNITS = np.ldexp(1.0, [0, 33, 0, 17])


def toy_case(seed=3, n=257):
    rng = np.random.default_rng(seed)
    s0 = [10.0 ** rng.uniform(-4.0, -2.0, n) for _ in range(4)]
    return G, s0


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("dt", [0.0, 1.0, 30.0, 300.0])
def test_toy_matches_the_closed_form(host, ft, dt):
    """r against (I − Δt M)⁻¹ M s formed in Float64, with M = D G D⁻¹ (entries over twenty orders of magnitude) and s = D s0, in the scaled unknowns r_j / c_j.
    The bound is reasoned, not observed: f = M s costs four roundings per row and no cancellation (≤ 4 eps of the row), an entry of A one fma (eps / 2), the
    solve a backward error of a few eps, and the forward error is κ∞(B) times their sum: (8 κ∞(B) + 4) eps, with κ∞ of the equilibrated matrix."""
    G_, s0 = toy_case()
    M = G_ * UNITS[:, None] / UNITS[None, :]
    s = [c * u for c, u in zip(s0, UNITS)]
    r, tend, rc = toy(host, ft, M, s, dt)
    assert rc == _abi.CMX_OK and np.isfinite(r).all()
    # the closed form is solved in the units of G, where LAPACK's own Float64 error is small, and carried over exactly: M = D G D⁻¹ and s = D s0 hold in
    # every bit (D: powers of two), so the solution is D times that of (G, s0)
    ref, _ = closed_form(ft, G_, s0, dt)
    ref, A = ref * UNITS[None, :], closed_form(ft, M, s, dt)[1]
    c = IC.column_scales(np.asarray(s, dtype=NPT[ft]))
    _, kappa = IC.equilibrated(np.broadcast_to(A, (c.shape[0], 4, 4)), c)
    err = IC.forward_error(r.T, ref, c)
    print(f"toy {ft} dt={dt}: worst forward error {err.max() / IC.EPS[ft]:.3g} eps, κ∞ ≤ {kappa.max():.3g}")
    assert (err <= (8.0 * kappa + 4.0) * IC.EPS[ft]).all(), (err.max() / IC.EPS[ft], kappa.max())
    if dt == 0.0:
        assert _same_bits(r, tend)


@pytest.mark.parametrize("ft", FTS)
def test_toy_units_do_not_change_the_solve(host, ft):
    """The same system in other units — M' = D M D⁻¹, s' = D s with D powers of two over ten orders of magnitude — is the same equilibrated system: r' = D r in
    every bit, for every tangent width."""
    G_, s0 = toy_case()
    for dt in (1.0, 30.0, 300.0):
        r0, _, _ = toy(host, ft, G_, s0, dt)
        for k in (1, 2, 4):
            r1, _, rc = toy(host, ft, G_ * UNITS[:, None] / UNITS[None, :], [c * u for c, u in zip(s0, UNITS)], dt, k=k)
            assert rc == _abi.CMX_OK
            assert _same_bits(r1, (r0.astype(np.float64) * UNITS[:, None]).astype(NPT[ft])), (dt, k)


@pytest.mark.parametrize("ft", FTS)
def test_toy_needs_the_pivot_search(host, ft):
    """Δt M_00 = 1 makes the leading entry of I − Δt M an exact zero — elimination without a row exchange divides by it — and the second column's largest
    entry sits in the last row: both exchanges are taken.  Against the closed form in the bound of test_toy_matches_the_closed_form."""
    M = np.array([[1.0, 0.5, -0.25, 0.125], [-0.5, 0.25, 0.5, -0.125], [0.25, -0.125, -0.5, 0.5], [0.125, -2.0, 0.25, -0.25]])
    rng = np.random.default_rng(5)
    s = [rng.uniform(1.0, 2.0, 65) for _ in range(4)]
    r, _, rc = toy(host, ft, M, s, 1.0)
    ref, A = closed_form(ft, M, s, 1.0)
    assert rc == _abi.CMX_OK and A[0, 0] == 0.0 and np.isfinite(r).all()
    c = IC.column_scales(np.asarray(s, dtype=NPT[ft]))
    _, kappa = IC.equilibrated(np.broadcast_to(A, (c.shape[0], 4, 4)), c)
    err = IC.forward_error(r.T, ref, c)
    assert (err <= (8.0 * kappa + 4.0) * IC.EPS[ft]).all(), (err.max() / IC.EPS[ft], kappa.max())


@pytest.mark.parametrize("ft", FTS)
def test_toy_singular_system_and_nan_rule(host, ft):
    """I − Δt M = 0 (M = I, Δt = 1): non-finite r at every point, no status.  A NaN in any input of a point — ρ included — gives NaN in every output of
    that point and in no other."""
    s = [np.full(4, 1.5) for _ in range(4)]
    r, tend, rc = toy(host, ft, np.eye(4), s, 1.0)
    assert rc == _abi.CMX_OK and not np.isfinite(r).any() and _same_bits(tend, np.full((4, 4), 1.5, dtype=NPT[ft]))
    G_, s0 = toy_case(n=9)
    clean, ctend, _ = toy(host, ft, G_, s0, 30.0)
    for j in range(5):
        cols = [np.ones(9)] + [c.copy() for c in s0]
        cols[j][4] = np.nan
        r, tend, _ = toy(host, ft, G_, cols[1:], 30.0, rho=cols[0])
        keep = np.arange(9) != 4
        assert np.isnan(r[:, 4]).all() and np.isnan(tend[:, 4]).all(), j
        assert _same_bits(r[:, keep], clean[:, keep]) and _same_bits(tend[:, keep], ctend[:, keep]), j


# ---- the two real schemes ---------------------------------------------------------------------------------------------------------------------------
# (scheme, parameter case): SB2006 (limited, perturbed exponents → the general-exponent instantiation), 1-moment the cases of tests/jacobian_1m_cases.py
SCHEMES = [("sb2006", (True, False)), ("sb2006", (False, False)), ("sb2006", (True, True)), ("mp1m", "default"), ("mp1m", "alt")]


def setup(oracle, scheme, case, ft):
    """(head, cols) of a scheme's parameter case."""
    if scheme == "sb2006":
        limited, perturbed = case
        wr = JC.warm_rain_params(ft, limited, JC.perturbed_overrides() if perturbed else None)
        return (wr, IC.head_sb2006(ft, wr, limited)), IC.sb2006_states(oracle)
    mp = J1.params(ft, case)
    return (mp, IC.head_mp1m(ft, mp)), IC.mp1m_states(oracle)


def jacobian_block(derivatives, scheme, ft, head, cols):
    """(J [4, 4, n] with respect to the species, f [4, n]) of the host build of the Jacobian entry, same float type."""
    wrt_all = _abi.SB2006_JAC_WRT if scheme == "sb2006" else _abi.MP1M_JAC_WRT
    J, f, rc = JH.host_jacobian(derivatives, scheme, ft, head, cols, wrt_all, IC.SPECIES[scheme])
    assert rc >= 0
    return J, f


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("scheme,case", SCHEMES)
def test_tendencies_and_dt_zero_are_the_plain_instantiation_bit_for_bit(host, derivatives, oracle, scheme, case, ft):
    """The `tendencies` output equals host_<scheme>_plain in every bit for every Δt and every tangent width, and so does r at Δt = 0."""
    (_, head), cols = setup(oracle, scheme, case, ft)
    plain, rc = JH.host_plain(derivatives, scheme, ft, head, cols)
    assert rc >= 0
    for dt in IC.DTS:
        for k in (0, 1, 2, 4):
            r, tend, rc = IC.host_implicit(host, scheme, ft, head, dt, cols, k=k)
            assert rc == _abi.CMX_OK
            assert _same_bits(tend, plain), (dt, k)
            if dt == 0.0:
                assert _same_bits(r, plain), k


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("scheme,case", SCHEMES)
def test_r_does_not_depend_on_the_tangent_width_or_the_selection(host, oracle, scheme, case, ft):
    """The seeds are run-time values and every tangent is computed by the same operations whatever K is (tests/test_sb2006_jacobian_host.py asserts it for
    the columns), so r is the same in every bit for K = 1, 2, 4; a requested subset of columns equals the same columns of the full call, and a call
    without `tendencies` gives the same r."""
    (_, head), cols = setup(oracle, scheme, case, ft)
    for dt in IC.DTS[1:]:
        full, _, _ = IC.host_implicit(host, scheme, ft, head, dt, cols, k=1)
        for k in (2, 4):
            r, _, rc = IC.host_implicit(host, scheme, ft, head, dt, cols, k=k)
            assert rc == _abi.CMX_OK and _same_bits(r, full), (dt, k)
    for null in [(0,), (1, 3), (0, 1, 2)]:
        r, tend, rc = IC.host_implicit(host, scheme, ft, head, 30.0, cols, null=null, with_tendencies=False, sentinel=7.0)
        full, _, _ = IC.host_implicit(host, scheme, ft, head, 30.0, cols)
        got = [q for q in range(4) if q not in null]
        assert rc == _abi.CMX_OK and tend is None and _same_bits(r[got], full[got]) and (r[list(null)] == 7.0).all(), null


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("scheme,case", SCHEMES)
def test_backward_error_against_lapack_in_the_same_precision(host, derivatives, oracle, scheme, case, ft):
    """ω of the fused solve, with J and f of the host Jacobian in the same float type, against numpy.linalg.solve on copies of the same A and f in that type:
    the worst ω over the set at most 4 × LAPACK's worst, and never required below 16 eps (implicit_cases)."""
    (_, head), cols = setup(oracle, scheme, case, ft)
    J, f = jacobian_block(derivatives, scheme, ft, head, cols)
    for dt in IC.DTS:
        r, _, rc = IC.host_implicit(host, scheme, ft, head, dt, cols)
        assert rc == _abi.CMX_OK and np.isfinite(r).all(), dt
        A, f64 = IC.system(ft, J, f, dt)
        bound, w_lapack = IC.omega_bound(ft, A, f64)
        w = float(IC.omega(A, r.T, f64).max())
        print(f"{scheme} {case} {ft} dt={dt}: worst ω fused {w:.3g} | LAPACK {w_lapack:.3g} (bound {bound:.3g})")
        assert w <= bound, (dt, w, w_lapack)


@pytest.mark.parametrize("scheme,case", SCHEMES)
def test_forward_error_against_the_float64_solve(host, derivatives, oracle, scheme, case):
    """Float64: r against numpy.linalg.solve in Float64 on the host-build Jacobian, in the scaled unknowns; 8 κ∞(B) eps per point with κ∞ of the equilibrated matrix;
    points with κ∞ > 1e6 are left out, at most 5 % of the set (asserted from the reference solve's matrices alone, for every Δt of the set)."""
    (_, head), cols = setup(oracle, scheme, case, "f64")
    J, f = jacobian_block(derivatives, scheme, "f64", head, cols)
    c = IC.column_scales(cols[3:7])
    for dt in IC.DTS:
        A, f64 = IC.system("f64", J, f, dt)
        B, kappa, rs = IC.equilibrated(A, c, with_row_scales=True)
        kept = kappa <= IC.KAPPA_MAX
        assert (~kept).mean() <= IC.MAX_LEFT_OUT, (dt, (~kept).mean())
        r, _, _ = IC.host_implicit(host, scheme, "f64", head, dt, cols)
        # the reference solve is handed the SAME system in its equilibrated form B z = D_r f, r* = D_c z (exact powers of two): on the raw A, whose rows
        # differ by ten orders of magnitude, LAPACK's own Float64 backward error is 1e-9 (test_backward_error_…) and it is no reference
        r_ref = np.linalg.solve(B, (f64 * rs)[..., None])[..., 0] * c
        err = IC.forward_error(r.T, r_ref, c)
        ratio = err[kept] / (kappa[kept] * IC.EPS["f64"])
        print(f"{scheme} {case} dt={dt}: left out {(~kept).mean():.2%}, largest κ∞ kept {kappa[kept].max():.3g}, worst error / (κ∞ eps) {ratio.max():.3g}")
        assert (ratio <= 8.0).all(), (dt, ratio.max())


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("scheme", ["sb2006", "mp1m"])
def test_nan_rule_and_absent_species(host, derivatives, oracle, scheme, ft):
    """A NaN in any of the seven inputs of a point gives NaN in all eight outputs of that point and changes no other point; the 1-moment Float64 entry does
    the same for ρ ≤ 0.  An absent species (input 0 or negative) has a zero Jacobian column — the column of A is the unit vector — and r is finite."""
    case = (True, False) if scheme == "sb2006" else "default"
    (_, head), cols = setup(oracle, scheme, case, ft)
    cols = [c[-16:].copy() for c in cols]
    clean, ctend, _ = IC.host_implicit(host, scheme, ft, head, 30.0, cols)
    bad_values = [(j, np.nan) for j in range(7)] + ([(0, 0.0), (0, -1.0)] if (scheme, ft) == ("mp1m", "f64") else [])
    for j, v in bad_values:
        bad = [c.copy() for c in cols]
        bad[j][5] = v
        r, tend, _ = IC.host_implicit(host, scheme, ft, head, 30.0, bad)
        keep = np.arange(16) != 5
        assert np.isnan(r[:, 5]).all() and np.isnan(tend[:, 5]).all(), (j, v)
        assert _same_bits(r[:, keep], clean[:, keep]) and _same_bits(tend[:, keep], ctend[:, keep]), (j, v)
    for absent in [(3,), (5, 6), (4,)] if scheme == "sb2006" else [(3,), (4, 6), (5,)]:
        gone = [c.copy() for c in cols]
        for j in absent:
            gone[j][:] = 0.0
            gone[j][::2] = -1e-9
        J, _ = jacobian_block(derivatives, scheme, ft, head, gone)
        for dt in IC.DTS:
            r, _, _ = IC.host_implicit(host, scheme, ft, head, dt, gone)
            assert np.isfinite(r).all(), (absent, dt)
        assert all((J[:, j - 3] == 0).all() for j in absent), absent


# ---- the device entries' argument statuses (no launch is reached) -------------------------------------------------------------------------------------
def test_argument_statuses_without_gpu():
    lib = _lib.lib()
    BAD, OK, UNSUPPORTED = _abi.CMX_ERR_BAD_ARG, _abi.CMX_OK, _abi.CMX_ERR_UNSUPPORTED
    cols, table = [C.c_void_p(4096)] * 7, (C.c_void_p * 4)(*[4096 + 64 * k for k in range(4)])
    empty = (C.c_void_p * 4)()
    huge = 16 * 0x7fffffff + 1
    for sfx in ("f32", "f64"):
        tps = P.ThermodynamicsParameters(sfx)
        wr, mp = P.WarmRainParams2M(sfx), P.Microphysics1MParams(sfx)
        for f, p, flags in ((getattr(lib, f"cmx_sb2006_warm_rain_implicit_tendencies_{sfx}"), wr.c, 1), (getattr(lib, f"cmx_mp1m_implicit_tendencies_{sfx}"), mp.c, mp.flags)):
            call = lambda *a: f(C.byref(p), C.byref(tps), flags, *a)      # noqa: E731
            assert f(None, C.byref(tps), flags, 10, *cols, 1.0, table, None, None) == BAD
            assert f(C.byref(p), None, flags, 10, *cols, 1.0, table, None, None) == BAD
            assert call(-1, *cols, 1.0, table, None, None) == BAD
            assert call(10, *([None] * 7), 1.0, table, None, None) == BAD                 # NULL columns
            assert call(10, *cols[:6], None, 1.0, table, None, None) == BAD
            assert call(10, *cols, 1.0, None, None, None) == BAD                          # `implicit` NULL itself
            assert call(10, *cols, 1.0, None, table, None) == BAD                         # … even with tendencies requested
            assert call(10, *cols, 1.0, empty, None, None) == BAD                         # no output column at all
            assert call(10, *cols, 1.0, empty, empty, None) == BAD
            for dt in (-1.0, -0.5e-300, float("nan"), float("inf"), float("-inf")):
                assert call(10, *cols, dt, table, table, None) == BAD, dt
            # the order: the count rule and n = 0 come first, as in the Jacobian entry of the scheme; Δt is checked after the columns
            assert call(huge, *cols, -1.0, None, None, None) == UNSUPPORTED
            assert call(0, *([None] * 7), -1.0, None, None, None) == OK
            assert call(0, *cols, float("nan"), table, None, None) == OK
        f1 = getattr(lib, f"cmx_mp1m_implicit_tendencies_{sfx}")
        assert f1(C.byref(mp.c), C.byref(tps), 1 << 17, 0, *cols, 1.0, table, None, None) == BAD      # the flags come before n = 0 there
        fs = getattr(lib, f"cmx_sb2006_warm_rain_implicit_tendencies_{sfx}")
        assert fs(C.byref(wr.c), C.byref(tps), 4, 0, *cols, 1.0, table, None, None) == OK               # … and after the columns here
