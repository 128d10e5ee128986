"""The derivatives of the SB2006 column step with respect to the PARAMETERS (include/cmx.h §26) in the HOST build tests/native/column_param_host.cpp — the header
the device kernels run (csrc/cmx_sb2006_column_param.hpp) and the host folds with tangents (cmx_sb2006.hpp, cmx_param_tangent.hpp) over columns on the CPU, so
the mathematics is tested without a GPU.  Names, reference (central differences of the Float64 oracle's column step, one ClimaParams name at a time), measure and
the 1 % condition: tests/column_param_cases.py.  tests/test_column_param_gpu.py repeats the assertions through the C ABI on the device."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import column_param_cases as KC
import column_products_cases as CC
from column_param_cases import CASE_IDS, CASES, MAIN_CASE, NAMES, host  # noqa: F401
from jacobian_host_build import REPO, _build, _same_bits
from cmx import _abi
from cmx import parameters as P

FTS = ["f64", "f32"]
NO_EXP = tuple(k for k in NAMES if k not in KC.EXPONENTS)
BAD, UNSUPPORTED = _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED


def _call(host, ft, case, shape="n7", names=NAMES, **kw):
    ref = KC.reference(case, shape)
    *structs, tables = KC.directions(ft, case, names)
    return ref, structs, tables, KC.host_jvp(host, ft, case, structs, ref["inv_dz"], ref["cols"], tables, **kw)


# ---- the host folds ---------------------------------------------------------------------------------------------------------------------------------
def test_digamma(host):
    """ψ of cmx_param_tangent.hpp against central differences of lgamma (their error is ≈ 1e-10 at h = 1e-5·x) and against cmx.parameters._digamma."""
    host.host_digamma.restype = C.c_double
    for x in (0.05, 0.3, 1.0, 1.5, 2.0 / 3.0, 3.0, 5.999, 6.0, 6.5, 17.0, 123.4):
        got = host.host_digamma(C.c_double(x))
        h = 1e-5 * x
        fd = (math.lgamma(x + h) - math.lgamma(x - h)) / (2 * h)
        assert abs(got - fd) <= 1e-7 * max(1.0, abs(fd)), (x, got, fd)
        assert abs(got - P._digamma(x)) <= 1e-12 * max(1.0, abs(got)), (x, got, P._digamma(x))
    assert math.isnan(host.host_digamma(C.c_double(0.0))) and math.isnan(host.host_digamma(C.c_double(-1.5)))
    # −γ: the series is cut after B₁₄, the first omitted term at x = 6 is B₁₆/(16·6¹⁶) = 1.6e-13; with the rounding of the five recurrence steps, 3e-13
    assert abs(host.host_digamma(C.c_double(1.0)) + 0.5772156649015329) < 3e-13


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("vel", CC.VELS)
@pytest.mark.parametrize("cloud", [False, True])
def test_the_value_parts_of_the_fold_with_tangents_are_the_plain_fold(host, ft, vel, cloud):
    """Every constant of SbConsts and CloudVelConsts — the fall-speed block and the fitted Chen-2022 coefficients included — bit for bit."""
    wr, tps, v, stokes = KC.params(ft, (True, vel, cloud))
    fn = getattr(host, f"host_column_plain_consts_{ft}")
    fn.restype = C.c_int32
    head = (C.byref(wr.c), C.byref(tps), C.byref(v), C.byref(stokes) if stokes is not None else None)
    n = fn(*head, 0, None)
    a, b = (C.c_ubyte * n)(), (C.c_ubyte * n)()
    assert fn(*head, 0, a) == n and fn(*head, 1, b) == n
    assert bytes(a) == bytes(b) and any(bytes(a))


def test_the_tangents_of_the_fall_speed_constants_follow_the_constructors(host):
    """ċ of the fold against central differences of the fold's own value parts with all four structs rebuilt from the overridden dictionary, for the names
    that reach the fall-speed constants; every tangent of the Chen-2022 constants is exactly zero."""
    fn = host.host_column_param_consts_f64
    fn.restype = C.c_int32
    case = (False, "sb", True)

    def fold(ov, direction=None):
        wr, tps, vel, stokes = KC.params("f64", case, ov)
        n = fn(C.byref(wr.c), C.byref(tps), C.byref(vel), C.byref(stokes), None, None, None, None, None)
        out = np.zeros(2 * n)
        d = [C.byref(s) for s in direction] if direction is not None else [None] * 4
        assert fn(C.byref(wr.c), C.byref(tps), C.byref(vel), C.byref(stokes), *d, out.ctypes.data_as(C.POINTER(C.c_double))) == n
        return out[:n], out[n:]
    wr = KC.params("f64", case)[0]
    base, zero = fold({})
    assert not zero.any()
    moved = np.zeros(base.size, bool)
    for name in KC.NEW_NAMES + ("SB2006_reference_air_density", "density_liquid_water", "kinematic_viscosity_of_air", "SB2006_cloud_gamma_distribution_coeff_nu",
                               "SB2006_cloud_gamma_distribution_coeff_mu"):
        t = P.DEFAULT_PARAMETERS[name]
        v, d = fold({}, P.column_parameter_direction(wr, {name: 1.0}))
        assert _same_bits(v, base)
        h = 1e-6 * abs(t)
        fd = (fold({name: t + h})[0] - fold({name: t - h})[0]) / (2 * h)
        scale = np.abs(base) / abs(t)
        assert (np.abs(d - fd) <= 1e-6 * scale + 1e-300).all(), (name, np.nonzero(np.abs(d - fd) > 1e-6 * scale)[0])
        moved |= d != 0
    # vel_s, aR, bR, cR, rc2, e_rc2cR and the four cloud constants all moved with some name; the Chen block (the 13 scalars and ChenLog behind) did not
    first_vel = 79 - 6
    assert moved[first_vel:first_vel + 6].all() and moved[-4:].all() and not moved[first_vel + 6:-4].any()


# ---- the reference alone ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_oracle_alone_stays_under_the_cap(oracle, case):
    ref = KC.reference_unchecked(case, "n7")
    pts, cls = KC.set_aside_shares(ref)
    print(f"{case} n7: set aside {pts:.4f} of the points, {cls:.4f} of the columns, worst h-vs-4h disagreement among the kept {ref['worst']:.3g}")
    assert pts <= KC.MAX_SET_ASIDE and cls <= KC.MAX_SET_ASIDE
    live = [NAMES[p] for p in range(len(NAMES)) if not ref["deadp"][p]]
    assert "density_liquid_water" in live and ("SB2006_raindrops_terminal_velocity_coeff_aR" in live) == (case[1] == "sb")
    if case == MAIN_CASE:
        for shape in ("n1", "n2", "n3"):
            assert KC.set_aside_shares(KC.reference_unchecked(case, shape)) == (0.0, 0.0), shape


# ---- J_θ δθ against the differenced oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_jvp_matches_the_differenced_oracle(host, oracle, ft, case):
    """LIMITED on and off, every velocity kind, cloud sedimentation on and off; the dead parameters of a case are exact zeros: aR, bR and cR under
    CMX_VEL_CHEN2022, the gravitational acceleration without cloud_vel, the T-only thermodynamic names in the precipitation row."""
    ref, structs, tables, (jv, jp, _, _, rc) = _call(host, ft, case)
    assert rc == KC.VEL_KIND[case[1]]
    KC.assert_parity(ft, ref, jv, jp, "host")
    idx = {k: NAMES.index(k) for k in NAMES}
    if case[1] != "sb":
        for k in KC.NEW_NAMES[:3]:
            assert not jv[idx[k]].any() and not jp[idx[k]].any(), k
    if not case[2]:
        assert not jv[idx["gravitational_acceleration"]].any() and not jp[idx["gravitational_acceleration"]].any()
    else:
        assert jv[idx["gravitational_acceleration"]].any()
    for k in ("latent_heat_vaporization_at_reference", "isobaric_specific_heat_liquid", "temperature_triple_point", "pressure_triple_point",
              "thermal_conductivity_of_air", "diffusivity_of_water_vapor", "condensation_evaporation_timescale"):
        assert not jp[idx[k]].any() and jv[idx[k]].any(), k


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("shape", ["n1", "n2", "n3"])
def test_small_columns(host, oracle, ft, shape):
    ref, structs, tables, (jv, jp, _, _, _) = _call(host, ft, MAIN_CASE, shape)
    KC.assert_parity(ft, ref, jv, jp, "host")


def test_the_measure_rejects_wrong_derivatives(host, oracle):
    """The fall-speed tangents left out (inv_dz = 0 in the place of the column's), a flux term with the wrong sign and the precipitation row of the level above
    all miss the bound."""
    ref, structs, tables, (jv, jp, _, _, _) = _call(host, "f64", MAIN_CASE)
    pointwise = KC.host_jvp(host, "f64", MAIN_CASE, structs, 0 * ref["inv_dz"], ref["cols"], tables)[0]
    for wrong, wrongp in ((pointwise, jp), (2 * pointwise - jv, jp), (jv, -jp), (jv, 0 * jp)):
        with pytest.raises(AssertionError):
            KC.assert_parity("f64", ref, wrong, wrongp, "wrong", report=False)


# ---- bit identities ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_value_parts_are_the_plain_column_step(host, oracle, ft, case):
    """Requested tendencies and precipitation flux of both entries equal the plain instantiation's (tests/native/column_products_host.cpp: the operations of
    the primal kernel), bit for bit, when no direction touches an exponent."""
    ref, structs, tables, (_, _, tend, pr, _) = _call(host, ft, case, names=NO_EXP)
    want, wantp, _ = CC.host_plain(_build("column_products_host"), ft, case, ref["inv_dz"], ref["cols"])
    assert _same_bits(tend, want) and _same_bits(pr, wantp)
    g, pbar = KC.cotangents(ref)
    _, tend2, pr2, rc = KC.host_vjp(host, ft, case, structs, ref["inv_dz"], ref["cols"], g, pbar, tables, ndir=3, with_primal=True)
    assert rc >= 0 and _same_bits(tend2, want) and _same_bits(pr2, wantp)


@pytest.mark.parametrize("ft", FTS)
def test_a_column_does_not_depend_on_ndir_or_on_the_split(host, oracle, ft):
    """1, KP, KP + 1 and 16 directions per call, and 1 … 4 directions per evaluation: the same bits."""
    ref, structs, tables, (full, fullp, _, _, _) = _call(host, ft, MAIN_CASE, names=NAMES[:16])
    kdev = getattr(host, f"host_column_param_k_{ft}")(1)
    args = (host, ft, MAIN_CASE, structs, ref["inv_dz"], ref["cols"], tables)
    for kp in (1, 2, 3, 4):
        jv, jp, _, _, rc = KC.host_jvp(*args, kp=kp)
        assert rc >= 0 and _same_bits(jv, full) and _same_bits(jp, fullp), kp
    for lo, nd in ((0, 1), (5, 1), (0, kdev), (3, kdev), (0, kdev + 1), (7, kdev + 1), (15, 1)):
        jv, jp, _, _, _ = KC.host_jvp(*args, lo=lo, ndir=nd, with_primal=False)
        assert _same_bits(jv[:nd], full[lo:lo + nd]) and _same_bits(jp[:nd], fullp[lo:lo + nd]), (lo, nd)
    g, pbar = KC.cotangents(ref)
    gfull = KC.host_vjp(*args[:6], g, pbar, tables)[0]
    for kp in (1, 2, 3, 4):
        assert _same_bits(KC.host_vjp(*args[:6], g, pbar, tables, kp=kp)[0], gfull), kp
    for lo, nd in ((0, 1), (0, kdev + 1), (9, 3)):
        assert _same_bits(KC.host_vjp(*args[:6], g, pbar, tables, lo=lo, ndir=nd)[0][:nd], gfull[lo:lo + nd]), (lo, nd)


@pytest.mark.parametrize("ft", FTS)
def test_linearity_in_the_direction(host, oracle, ft):
    """J(a δ₁ + b δ₂) = a J δ₁ + b J δ₂ to 4 eps of the row scale (the tangents are linear forms evaluated in the float type)."""
    ref = KC.reference(MAIN_CASE, "n2")
    wr, tps, vel, stokes = structs = KC.params(ft, MAIN_CASE)
    th = dict(zip(NAMES, KC.theta()))
    n1, n2 = "SB2006_raindrops_terminal_velocity_coeff_cR", "density_liquid_water"
    a, b = 0.625, -0.375      # |a| + |b| = 1: the terms of the identity stay within the row scale the bound is stated in
    quads = [P.column_parameter_direction(wr, w) for w in ({n1: th[n1]}, {n2: th[n2]}, {n1: a * th[n1], n2: b * th[n2]})]
    tables = [(type(quads[0][k]) * 3)(*[q[k] for q in quads]) for k in range(4)]
    jv, jp, _, _, rc = KC.host_jvp(host, ft, MAIN_CASE, structs, ref["inv_dz"], ref["cols"], tables)
    assert rc >= 0
    eps = np.finfo(KC.NPT[ft]).eps
    for y, scale in ((jv.astype(np.float64), np.abs(ref["S"]).max(axis=1)), (jp.astype(np.float64)[:, None], np.abs(ref["Sp"]).max(axis=1))):      # the row scale s_o
        used = np.max(np.abs(y[2] - (a * y[0] + b * y[1])) / np.where(scale > 0, scale, 1.0)) / eps
        print(f"{ft}: linearity, worst difference {used:.3g} eps of the row scale")
        assert (np.abs(y[2] - (a * y[0] + b * y[1])) <= 4 * eps * scale).all(), used


# ---- the gradient -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", [MAIN_CASE, (False, "chen", True), (True, "chen_gen", False)], ids=["main", "notlimited-chen-cloud", "limited-chen_gen-nocloud"])
def test_the_gradient_is_the_sum_over_the_jvp_columns(host, oracle, ft, case):
    """grad[d] against Σ ḡ·jvp_d + Σ p̄·ṗ_d summed in float64 from the jvp columns: the per-point sums differ by the rounding of a chain of at most eight fma in
    the float type, so |difference| ≤ 8 eps·Σ |terms| (the bound of the §22 gradient tests)."""
    ref, structs, tables, (jv, jp, _, _, _) = _call(host, ft, case)
    g, pbar = KC.cotangents(ref)
    grad, _, _, rc = KC.host_vjp(host, ft, case, structs, ref["inv_dz"], ref["cols"], g, pbar, tables)
    assert rc == KC.VEL_KIND[case[1]]
    gq, pq = np.asarray(g, dtype=KC.NPT[ft]), np.asarray(pbar, dtype=KC.NPT[ft])
    want, size = KC.grad_from_jvp(gq, pq, jv, jp)
    eps = np.finfo(KC.NPT[ft]).eps
    assert (np.abs(grad - want) <= 8 * eps * size).all(), np.max(np.abs(grad - want) / np.where(size > 0, size, 1))
    assert ((size == 0) == (grad == 0)).all()
    # without cotangents at all: exact +0; the precipitation cotangent alone reaches the gradient
    zero = KC.host_vjp(host, ft, case, structs, ref["inv_dz"], ref["cols"], None, None, tables)[0]
    assert not zero.any() and not np.signbit(zero).any()
    only_p = KC.host_vjp(host, ft, case, structs, ref["inv_dz"], ref["cols"], None, pbar, tables)[0]
    wantp, sizep = KC.grad_from_jvp(0 * gq, pq, jv, jp)
    assert (np.abs(only_p - wantp) <= 8 * eps * sizep).all() and only_p.any()


# ---- the NaN rule and the argument checks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_the_nan_rule(host, oracle, ft):
    """A NaN in a state input → every output of that point; in an input of the fluxes → also the cell below and, from level 0, the precipitation outputs; in
    the gradient any of them, or a NaN cotangent, makes every grad[d] NaN.  No other point changes, bit for bit."""
    names = NO_EXP[:5] + KC.NEW_NAMES
    ref, structs, tables, (cjv, cjp, ctend, cpr, _) = _call(host, ft, MAIN_CASE, "n2", names=names)
    n_col, n_lev = ref["n_col"], ref["n_lev"]
    args = (host, ft, MAIN_CASE, structs, ref["inv_dz"])
    g, pbar = KC.cotangents(ref)
    i_top, i_bot = 5 * n_lev + 1, 5 * n_lev
    others = ~np.isin(np.arange(n_col * n_lev), (i_top, i_bot))
    for j in range(7):
        bad = [np.array(c) for c in ref["cols"]]
        bad[j][5, 1] = np.nan
        jv, jp, tend, pr, _ = KC.host_jvp(*args, bad, tables)
        assert np.isnan(jv[:, :, i_top]).all() and np.isnan(tend[:, i_top]).all(), j
        below = j in (0, 3, 4, 5, 6)
        assert np.isnan(jv[:, 2:, i_bot]).all() == below and np.isnan(tend[2:, i_bot]).all() == below, j
        assert not np.isnan(jp[:, 5]).any() and not np.isnan(pr[5]), j      # level 1 is not the surface: the precipitation flux is level 0's own
        assert _same_bits(jv[:, :, others], cjv[:, :, others]) and _same_bits(tend[:, others], ctend[:, others]), j
        assert np.isnan(KC.host_vjp(*args, bad, g, pbar, tables)[0]).all(), j
        bad = [np.array(c) for c in ref["cols"]]
        bad[j][5, 0] = np.nan
        jv, jp, tend, pr, _ = KC.host_jvp(*args, bad, tables)
        assert np.isnan(jp[:, 5]).all() == below and np.isnan(pr[5]) == below, j
        assert _same_bits(np.delete(jp, 5, axis=1), np.delete(cjp, 5, axis=1)) and _same_bits(jv[:, :, i_top], cjv[:, :, i_top]), j
    gb = [np.array(a) for a in g]
    gb[2][i_bot] = np.nan
    assert np.isnan(KC.host_vjp(*args, ref["cols"], gb, pbar, tables)[0]).all()
    pb = np.array(pbar)
    pb[3] = np.nan
    assert np.isnan(KC.host_vjp(*args, ref["cols"], g, pb, tables)[0]).all()


def test_argument_checks(host, oracle):
    ref, structs, tables, (jv, jp, _, _, rc) = _call(host, "f64", MAIN_CASE, "n3", names=NO_EXP[:3])
    args = (host, "f64", MAIN_CASE, structs, ref["inv_dz"], ref["cols"])
    g, pbar = KC.cotangents(ref)
    both = _abi.CMX_SB2006_LIMITED | _abi.CMX_VEL_SB2006 | _abi.CMX_VEL_CHEN2022
    for f in (both, _abi.CMX_SB2006_LIMITED, _abi.CMX_VEL_SB2006 | (1 << 9)):
        assert KC.host_jvp(*args, tables, override_flags=f)[-1] == BAD and KC.host_vjp(*args, g, pbar, tables, override_flags=f)[-1] == BAD
    assert KC.host_jvp(*args, tables, ndir=0)[-1] == BAD and KC.host_jvp(*args, tables, ndir=_abi.CMX_PARAM_MAX_DIRS + 1)[-1] == BAD
    assert KC.host_jvp(*args, tables, use=(False, True, True, True))[-1] == BAD                  # d_warm_rain is required
    # d_tps, d_vel, d_cloud_vel NULL: zero directions there
    wr = structs[0]
    quads = [P.column_parameter_direction(wr, {"SB2006_collection_kernel_coeff_kcc": 2.0})] * 2
    t2 = [(type(quads[0][k]) * 2)(*[q[k] for q in quads]) for k in range(4)]
    a = KC.host_jvp(*args, t2)
    b = KC.host_jvp(*args, t2, use=(True, False, False, False))
    assert b[-1] >= 0 and _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    # a non-finite component anywhere in a direction; a Chen-2022 component, whatever the flags
    for k, field in ((0, "condevap_tau_relax"), (1, "cp_v"), (3, "grav")):
        bad = [(type(t[0]) * 2)(*t) for t in t2]
        setattr(bad[k][1], field, float("inf"))
        assert KC.host_jvp(*args, bad)[-1] == BAD, field
    bad = [(type(t[0]) * 2)(*t) for t in t2]
    bad[2][1].sb2006.aR = float("nan")
    assert KC.host_jvp(*args, bad)[-1] == BAD
    for case in (MAIN_CASE, (True, "chen", True)):
        bad = [(type(t[0]) * 2)(*t) for t in t2]
        bad[2][1].chen2022.b_rho = 1e-3
        s = KC.params("f64", case)
        assert KC.host_jvp(host, "f64", case, s, ref["inv_dz"], ref["cols"], bad)[-1] == UNSUPPORTED
        assert KC.host_vjp(host, "f64", case, s, ref["inv_dz"], ref["cols"], g, pbar, bad)[-1] == UNSUPPORTED
    # without cloud_vel, d_cloud_vel is ignored: not read, not checked
    nocloud = (True, "sb", False)
    s = KC.params("f64", nocloud)
    bad = [(type(t[0]) * 2)(*t) for t in t2]
    bad[3][0].grav = float("nan")
    a = KC.host_jvp(host, "f64", nocloud, s, ref["inv_dz"], ref["cols"], bad)
    b = KC.host_jvp(host, "f64", nocloud, s, ref["inv_dz"], ref["cols"], t2, use=(True, True, True, False))
    assert a[-1] >= 0 and _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    # a direction on an exponent selects the general-exponent instantiation for the whole call: other columns keep their VALUES to rounding, not their bits
    names = NO_EXP[:2] + KC.EXPONENTS[:1]
    *s, te = KC.directions("f64", MAIN_CASE, names)
    with_exp = KC.host_jvp(*args[:3], s, ref["inv_dz"], ref["cols"], te)
    without = KC.host_jvp(*args[:3], s, ref["inv_dz"], ref["cols"], te, ndir=2)
    assert with_exp[-1] >= 0 and np.allclose(with_exp[0][:2], without[0][:2], rtol=1e-9, atol=0) and with_exp[0][2].any()
    # n_col = 0: CMX_OK, and the gradient entry writes zeros
    empty = [np.zeros((0, 3)) for _ in range(7)]
    assert KC.host_jvp(host, "f64", MAIN_CASE, structs, ref["inv_dz"], empty, tables)[-1] == 0
    grad, _, _, rc = KC.host_vjp(host, "f64", MAIN_CASE, structs, ref["inv_dz"], empty, None, None, tables)
    assert rc >= 0 and not grad.any()


# ---- the stand-alone program ------------------------------------------------------------------------------------------------------------------------
def test_the_stand_alone_program_runs(tmp_path):
    """tests/native/column_param_host.cpp with its own main (the program to build with host sanitizer flags): compiled plainly here, run on the default
    parameter structs written as raw bytes; it checks the gradient against the sum over the jvp columns itself."""
    exe = tmp_path / "column_param"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DCMX_COLUMN_PARAM_MAIN", "-o", str(exe),
                    str(REPO / "tests" / "native" / "column_param_host.cpp")], check=True)
    files = []
    for ft in ("f32", "f64"):
        wr, tps, vel, stokes = KC.params(ft, MAIN_CASE)
        path = tmp_path / f"params_{ft}.bin"
        path.write_bytes(b"".join(bytes(memoryview(s)) for s in (wr.c, tps, vel, stokes)))
        files.append(str(path))
    r = subprocess.run([str(exe), *files], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


def test_the_public_names_and_symbols():
    """The wrappers, their result tuples, the direction table and the four symbols of include/cmx.h §26."""
    import cmx
    from cmx import _lib
    assert cmx.ColumnParamJvp2M._fields == ("jvp", "jvp_precip", "tendencies", "precip_flux")
    assert cmx.ColumnParamVjp2M._fields == ("grad", "tendencies", "precip_flux", "wrt")
    assert callable(cmx.column_param_jvp_2m) and callable(cmx.column_param_vjp_2m)
    assert set(P.WARM_RAIN_2M_DIRECTION_FIELDS) < set(P.COLUMN_2M_DIRECTION_FIELDS) and set(KC.NEW_NAMES) <= set(P.COLUMN_2M_DIRECTION_FIELDS)
    for k, v in P.WARM_RAIN_2M_DIRECTION_FIELDS.items():
        assert P.COLUMN_2M_DIRECTION_FIELDS[k][:len(v)] == tuple(v), k
    for sfx in ("f32", "f64"):
        for product in ("jvp", "vjp"):
            assert getattr(_lib.lib(), f"cmx_sb2006_column_param_{product}_{sfx}").restype is C.c_int32
    wr = P.WarmRainParams2M("f64")
    d = P.column_parameter_direction(wr, {"density_liquid_water": 2.0, "gravitational_acceleration": 0.5})
    assert d[0].seifert_beheng.pdf_r.rho_w == 2.0 and d[3].rho_w == 2.0 and d[3].grav == 0.5 and d[2].sb2006.rho_w == 2.0 and d[1].R_v == 0.0
    with pytest.raises(ValueError):
        P.column_parameter_direction(wr, {"Chen2022_table_B1_coeff_b_rho": 1.0})
