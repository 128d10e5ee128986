"""The derivatives of the 1-moment column step with respect to the PARAMETERS (include/cmx.h §28) in the HOST build tests/native/column_param_1m_host.cpp — the
header the device kernels run (csrc/cmx_mp1m_column_param.hpp) and the host folds with tangents (cmx_mp1m.hpp, cmx_mp1m_vel.hpp, cmx_param_tangent.hpp) over
columns on the CPU, so the mathematics is tested without a GPU.  Names, reference (central differences of the Float64 oracle's column step, one name at a
time), measure and the 1 % condition: tests/column_param_1m_cases.py.  tests/test_column_param_1m_gpu.py repeats the assertions through the C ABI on the
device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import column_param_1m_cases as KC
import column_products_1m_cases as K1
from column_param_1m_cases import CASE_IDS, CASES, MAIN_CASE, WHICH, host  # noqa: F401
from jacobian_host_build import REPO, _build, _same_bits
from cmx import _abi
from cmx import parameters as P

FTS = ["f64", "f32"]
BAD, UNSUPPORTED = _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED


def no_exp(case):
    return tuple(k for k in KC.names(case) if k not in KC.EXPONENT_NAMES)


def _call(host, ft, case, which="cold", shape="n7", nm=None, **kw):
    ref = KC.reference(case, which, shape)
    structs, tables = KC.directions(ft, case, nm)
    return ref, structs, tables, KC.host_jvp(host, ft, structs, ref["inv_dz"], ref["cols"], tables, **kw)


def _sub(ref, nm):
    """The reference restricted to the names nm (for calls with a subset of the directions)."""
    idx = [ref["names"].index(k) for k in nm]
    return dict(ref, names=tuple(nm), S=ref["S"][:, idx], Sp=ref["Sp"][:, idx], S4=ref["S4"][:, idx], Sp4=ref["Sp4"][:, idx], dead=ref["dead"][idx],
                deadp=ref["deadp"][idx])


# ---- the host folds ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_value_parts_of_the_fold_with_tangents_are_the_plain_fold(host, ft, case):
    """Every folded constant the kernels receive — Mp1mConsts, the fall-speed constants, ε, b, b_ρ and the Γ polynomials — equals what the primal column
    entry folds (make_mp1m_consts, make_vel1m_consts, add_sedimentation_consts), bit for bit."""
    structs = KC.params(ft, case)
    fn = getattr(host, f"host_column_param_1m_plain_consts_{ft}")
    fn.restype = C.c_int32
    n = fn(*KC.head(structs), 0, None)
    a, b = np.zeros(n, dtype=KC.NPT[ft]), np.ones(n, dtype=KC.NPT[ft])
    assert fn(*KC.head(structs), 0, a.ctypes.data_as(C.POINTER(KC.CT[ft]))) == n and fn(*KC.head(structs), 1, b.ctypes.data_as(C.POINTER(KC.CT[ft]))) == n
    assert a.tobytes() == b.tobytes() and a.any()


def test_the_tangents_of_the_fall_speed_constants_follow_the_constructors(host):
    """ċ of the fold against central differences of the fold's own value parts with all five structs rebuilt from the overridden dictionary, for names that
    reach the fall-speed constants — Γ(C_l + 4) and Γ(F_l + 4) among them; every value part is the zero direction's, bit for bit."""
    fn = host.host_column_param_1m_consts_f64
    fn.restype = C.c_int32
    npt = host.host_column_param_1m_point_consts()

    def fold(ov, direction=None):
        structs = KC.params("f64", MAIN_CASE, ov)
        n = fn(*KC.head(structs), None, None, None, None, None, None)
        out = np.zeros(2 * n)
        d = [C.byref(s) for s in direction] if direction is not None else [None] * 5
        assert fn(*KC.head(structs), *d, out.ctypes.data_as(C.POINTER(C.c_double))) == n
        return out[:n], out[n:]
    mp = KC.params("f64", MAIN_CASE)[0]
    base, zero = fold({})
    assert not zero.any()
    moved = np.zeros(base.size, bool)
    for name in KC.SEDIMENTATION_ONLY + ("density_liquid_water", "gravitational_acceleration", "kinematic_viscosity_of_air", "snow_apparent_density",
                                         "cloud_ice_apparent_density", "Chen2022_table_B5_Cl[0]", "Chen2022_table_B5_Fl[0]", "Chen2022_table_B5_Fl[1]",
                                         "Chen2022_table_B5_Gl[2]", "Chen2022_table_B5_Hl[1]", "Chen2022_table_B3_Cs[3]", "Chen2022_table_B3_Gs[1]",
                                         "Chen2022_table_B1_ai[1]", "Chen2022_table_B1_ai[2]", "Chen2022_table_B1_ci[1]", "Chen2022_table_B1_ci[2]",
                                         "Chen2022_table_B1_a3_pow_coeff", "snow_flake_size_distribution_coefficient_mu",
                                         "snow_flake_size_distribution_coefficient_nu", "rain_mass_size_relation_coefficient_me", "rain_drop_length_scale",
                                         "snow_mass_size_relation_coefficient_me", "snow_flake_length_scale"):
        t = KC._value({}, name)
        v, d = fold({}, P.column_parameter_direction_1m(mp, {name: 1.0}))
        assert _same_bits(v, base), name
        h = 1e-6 * abs(t)
        fd = (fold(KC.override_with(MAIN_CASE, name, t + h))[0] - fold(KC.override_with(MAIN_CASE, name, t - h))[0]) / (2 * h)
        scale = np.abs(base) / abs(t)
        assert (np.abs(d - fd) <= 2e-6 * scale + 1e-300).all(), (name, np.nonzero(np.abs(d - fd) > 2e-6 * scale)[0], d[np.abs(d - fd) > 2e-6 * scale],
                                                                  fd[np.abs(d - fd) > 2e-6 * scale])
        assert d.any(), name
        if name in KC.SEDIMENTATION_ONLY:
            assert not d[:npt].any(), name                                   # nothing of the point function moves
        moved |= d != 0
    # every fall-speed constant with a tangent moved with some name; c₁ of the rain table is 0 and has no step 1e-6·|θ|: its own tangent is the literal 1000
    c1 = 13
    assert moved[npt:][np.arange(moved.size - npt) != c1].all(), np.nonzero(~moved[npt:])[0]
    d = fold({}, P.column_parameter_direction_1m(mp, {"Chen2022_table_B1_ci[0]": 1.0}))[1]
    assert d[npt + c1] == 1000.0 and np.count_nonzero(d) == 1


def test_the_two_names_that_only_look_dead(host):
    """Chen2022_table_B5_Fl[2] and Hl[2]: the tangent of the fold is tiny and NOT zero, and the reference cannot see it."""
    ref = KC.reference(MAIN_CASE, "cold", "n7")
    structs = KC.params("f64", MAIN_CASE)
    fn = host.host_column_param_1m_consts_f64
    fn.restype = C.c_int32
    n = fn(*KC.head(structs), None, None, None, None, None, None)
    for name in KC.NOT_STRUCTURALLY_DEAD:
        p = ref["names"].index(name)
        assert ref["dead"][p] and ref["deadp"][p], name
        out = np.zeros(2 * n)
        d = P.column_parameter_direction_1m(structs[0], {name: KC._value({}, name)})
        assert fn(*KC.head(structs), *[C.byref(s) for s in d], out.ctypes.data_as(C.POINTER(C.c_double))) == n
        t = out[n:]
        assert np.count_nonzero(t) >= 1 and np.all(np.abs(t[t != 0]) < 1e-18 * np.abs(out[:n][t != 0])), (name, t[t != 0])


# ---- the reference alone ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_oracle_alone_stays_under_the_cap(oracle, case, which):
    ref = KC.reference(case, which, "n7")
    live = [ref["names"][p] for p in range(len(ref["names"])) if not ref["deadp"][p]]
    for k in ("snow_aspect_ratio", "snow_aspect_ratio_coefficient", "Chen2022_table_B1_q_coeff", "Chen2022_table_B1_ai[0]", "Chen2022_table_B5_Al[0]",
              "Chen2022_table_B5_Cl[1]", "density_liquid_water", "snow_apparent_density"):
        assert k in live, k
    for k in ("Chen2022_table_B3_As[0]", "cloud_liquid_sedimentation_number_concentration", "gravitational_acceleration"):      # cloud species: no surface flux
        assert k not in live and not ref["dead"][ref["names"].index(k)], k
    if case == MAIN_CASE:
        for shape in ("n1", "n2", "n3"):
            KC.reference(case, which, shape)


# ---- J_θ δθ against the differenced oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_jvp_matches_the_differenced_oracle(host, oracle, ft, case, which):
    """Every case and set on n7, every name of the case; with an exponent among the directions the run-time-flags instantiation serves the whole call."""
    ref, structs, tables, (jv, jp, _, _, rc) = _call(host, ft, case, which)
    assert rc == (KIND_RT := KC.KIND[case] & 2), (rc, KIND_RT)
    KC.assert_parity(ft, ref, jv, jp, "host")
    idx = {k: i for i, k in enumerate(ref["names"])}
    for k in KC.SEDIMENTATION_ONLY:
        assert jv[idx[k]].any(), k
    for k in ("Chen2022_table_B1_ai[0]", "Chen2022_table_B5_Al[0]", "snow_aspect_ratio"):
        assert jp[:, idx[k]].any(), k
    # thermodynamic names act on the point function only: dead in both precipitation rows, alive in the tendencies
    for k in ("latent_heat_vaporization_at_reference", "pressure_triple_point", "thermal_conductivity_of_air"):
        assert not jp[:, idx[k]].any() and jv[idx[k]].any(), k


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_instantiation_is_the_primal_entrys_without_a_direction_on_an_exponent(host, oracle, ft, case):
    nm = no_exp(case)
    ref, structs, tables, (jv, jp, _, _, rc) = _call(host, ft, case, "warm", nm=nm)
    assert rc == KC.KIND[case]
    KC.assert_parity(ft, _sub(ref, nm), jv, jp, "host without exponents")


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("shape", ["n1", "n2", "n3"])
def test_small_columns(host, oracle, ft, shape):
    for which in WHICH:
        ref, structs, tables, (jv, jp, _, _, _) = _call(host, ft, MAIN_CASE, which, shape)
        KC.assert_parity(ft, ref, jv, jp, "host")


def test_the_measure_rejects_wrong_derivatives(host, oracle):
    """The fall-speed tangents left out (inv_dz = 0 in the place of the column's), a flux term with the wrong sign and wrong precipitation rows all miss."""
    ref, structs, tables, (jv, jp, _, _, _) = _call(host, "f64", MAIN_CASE)
    pointwise = KC.host_jvp(host, "f64", structs, 0 * ref["inv_dz"], ref["cols"], tables)[0]
    for wrong, wrongp in ((pointwise, jp), (2 * pointwise - jv, jp), (jv, -jp), (jv, jp[::-1]), (jv, 0 * jp)):
        with pytest.raises(AssertionError):
            KC.assert_parity("f64", ref, wrong, wrongp, "wrong", report=False)


# ---- bit identities ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_value_parts_are_the_plain_column_step(host, oracle, ft, case):
    """Requested tendencies and precipitation fluxes of both entries equal the plain instantiation's (tests/native/column_products_1m_host.cpp: the
    operations of the primal kernel), bit for bit, when no direction moves an exponent."""
    nm = no_exp(case)[:20]
    ref, structs, tables, (_, _, tend, pr, rc) = _call(host, ft, case, nm=nm)
    assert rc == KC.KIND[case]
    want, wantp, _ = K1.host_plain(_build("column_products_1m_host"), ft, case, ref["inv_dz"], ref["cols"])
    assert _same_bits(tend, want) and _same_bits(pr, wantp)
    g, pbar = KC.cotangents(ref)
    _, tend2, pr2, rc = KC.host_vjp(host, ft, structs, ref["inv_dz"], ref["cols"], g, pbar, tables, ndir=3, with_primal=True)
    assert rc >= 0 and _same_bits(tend2, want) and _same_bits(pr2, wantp)


@pytest.mark.parametrize("ft", FTS)
def test_a_column_does_not_depend_on_ndir_or_on_the_split(host, oracle, ft):
    """1, KP, KP + 1 and 16 directions per call, 1 … 4 directions per evaluation, and more than CMX_PARAM_MAX_DIRS names split into calls: the same bits."""
    nm = no_exp(MAIN_CASE)
    ref, structs, tables, (full, fullp, _, _, _) = _call(host, ft, MAIN_CASE, nm=nm)
    kdev = getattr(host, f"host_column_param_1m_k_{ft}")(0)
    args = (host, ft, structs, ref["inv_dz"], ref["cols"], tables)
    for kp in (1, 2, 3, 4):
        jv, jp, _, _, rc = KC.host_jvp(*args, ndir=16, kp=kp)
        assert rc >= 0 and _same_bits(jv, full[:16]) and _same_bits(jp, fullp[:, :16]), kp
    for lo, nd in ((0, 1), (5, 1), (0, kdev), (3, kdev), (0, kdev + 1), (7, kdev + 1), (len(nm) - 1, 1), (40, 16)):
        jv, jp, _, _, _ = KC.host_jvp(*args, lo=lo, ndir=nd, with_primal=False)
        assert _same_bits(jv[:nd], full[lo:lo + nd]) and _same_bits(jp[:, :nd], fullp[:, lo:lo + nd]), (lo, nd)
    g, pbar = KC.cotangents(ref)
    gfull = KC.host_vjp(*args[:5], g, pbar, tables)[0]
    for kp in (1, 2, 3, 4):
        assert _same_bits(KC.host_vjp(*args[:5], g, pbar, tables, ndir=16, kp=kp)[0], gfull[:16]), kp
    for lo, nd in ((0, 1), (0, kdev + 1), (9, 3)):
        assert _same_bits(KC.host_vjp(*args[:5], g, pbar, tables, lo=lo, ndir=nd)[0][:nd], gfull[lo:lo + nd]), (lo, nd)


@pytest.mark.parametrize("ft", FTS)
def test_no_sedimentation_gives_the_point_functions_derivatives(host, oracle, ft):
    """inv_dz ≡ 0, directions on mp and tps only: the four jvp rows equal host_mp1m_param_jvp's (§23) under == wherever finite — here everywhere."""
    import param_1m_cases as P1
    nm = tuple(k for k in no_exp(MAIN_CASE) if k in P.MICROPHYSICS_1M_DIRECTION_NAMES)[:32]
    ref = KC.reference(MAIN_CASE, "cold", "n7")
    structs, tables = KC.directions(ft, MAIN_CASE, nm)
    jv, _, tend, _, rc = KC.host_jvp(host, ft, structs, 0 * ref["inv_dz"], ref["cols"], tables, use=(True, True, False, False, False))
    assert rc == KC.KIND[MAIN_CASE]
    ph = _build("param_derivatives_host")
    fn = getattr(ph, f"host_mp1m_param_jvp_{ft}")
    fn.restype = C.c_int32
    x = [KC._flat(ft, c) for c in ref["cols"]]
    n = x[0].size
    for p0 in range(0, len(nm), _abi.CMX_PARAM_MAX_DIRS):
        nd = min(_abi.CMX_PARAM_MAX_DIRS, len(nm) - p0)
        pv = np.full((nd, 4, n), -7.0, dtype=KC.NPT[ft])
        st = fn(C.byref(structs[0].c), C.byref(structs[1]), C.c_uint32(structs[0].flags), C.c_int(0), C.c_int64(n), KC._arr(ft, x), C.c_int32(nd),
                C.byref(tables[0][p0]), C.byref(tables[1][p0]), KC._arr(ft, [pv[d, o] for d in range(nd) for o in range(4)]), None)
        assert st >= 0
        fin = np.isfinite(jv[p0:p0 + nd])
        assert fin.all() and (jv[p0:p0 + nd] == pv).all()


@pytest.mark.parametrize("ft", FTS)
def test_the_euler_relation_of_the_rain_fall_speed(host, oracle, ft):
    """The rain fall speed is linear in chen_rain.a: for δa = a (all three entries) ṗ_rai = precip_rai, and the flux part of the rain row — the row minus the
    same row at inv_dz ≡ 0 — is the flux part of the rain tendency, to a few ulp of Σ |terms| (the three terms aₖ·(…) of the fall speed, of mixed sign, of
    the point and of the point above, and the two rounded tendencies whose difference the primal's flux part is)."""
    ref = KC.reference(MAIN_CASE, "warm", "n7")
    structs = KC.params(ft, MAIN_CASE)
    a = list(P.DEFAULT_PARAMETERS["Chen2022_table_B1_ai"])
    tables = KC.tables_of([P.column_parameter_direction_1m(structs[0], {f"Chen2022_table_B1_ai[{i}]": a[i] for i in range(3)})] +
                          [P.column_parameter_direction_1m(structs[0], {f"Chen2022_table_B1_ai[{i}]": a[i]}) for i in range(3)])
    jv, jp, tend, pr, rc = KC.host_jvp(host, ft, structs, ref["inv_dz"], ref["cols"], tables)
    jv0, _, tend0, _, _ = KC.host_jvp(host, ft, structs, 0 * ref["inv_dz"], ref["cols"], tables)
    assert rc >= 0 and not jv0.any()                                       # a acts through the rain flux only
    eps = np.finfo(KC.NPT[ft]).eps
    jp, pr, jv, tend, tend0 = (np.asarray(v, dtype=np.float64) for v in (jp, pr, jv, tend, tend0))
    terms = np.abs(jp[0, 1:]).sum(axis=0)                                   # Σ_k |a_k ∂p/∂a_k|
    assert (np.abs(jp[0, 0] - pr[0]) <= 8 * eps * terms).all(), np.max(np.abs(jp[0, 0] - pr[0]) / np.where(terms > 0, terms, 1)) / eps
    assert not jp[1].any()
    rai = _abi.MP1M_JAC_OUT.index("dq_rai_dt")
    # the sizes of what is added up: every level as a column of its own gives F and Ḟ of each point; the row's flux part is g·(Ḟ_above − Ḟ_own) per direction,
    # and the primal's is the difference of two rounded tendencies
    single = [np.asarray(c).reshape(-1, 1) for c in ref["cols"]]
    _, jp1, _, _, _ = KC.host_jvp(host, ft, structs, np.ones(1), single, tables)
    Fd = np.abs(np.asarray(jp1[0, 1:], dtype=np.float64)).sum(axis=0).reshape(ref["n_col"], ref["n_lev"])
    gk = ref["inv_dz"][None, :] / ref["cols"][0]
    up = np.zeros_like(Fd)
    up[:, :-1] = Fd[:, 1:]
    size = (gk * (Fd + up)).reshape(-1) + np.abs(tend[rai]) + np.abs(tend0[rai])
    flux = tend[rai] - tend0[rai]
    assert (np.abs(jv[0, rai] - flux) <= 8 * eps * size).all(), np.max(np.abs(jv[0, rai] - flux) / np.where(size > 0, size, 1)) / eps
    assert jv[0, rai].any() and not np.delete(jv[0], rai, axis=0).any()


# ---- the gradient -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_gradient_is_the_sum_over_the_jvp_columns(host, oracle, ft, case):
    """grad[d] against Σ ḡ·jvp_d + Σ p̄·ṗ_d summed in float64 from the jvp columns: within BOUND of the size of the terms; with the per-point chains of at most
    eight fma in the float type the difference is in fact a few eps."""
    ref, structs, tables, (jv, jp, _, _, _) = _call(host, ft, case)
    g, pbar = KC.cotangents(ref)
    grad, _, _, rc = KC.host_vjp(host, ft, structs, ref["inv_dz"], ref["cols"], g, pbar, tables)
    assert rc == KC.KIND[case] & 2
    gq, pq = np.asarray(g, dtype=KC.NPT[ft]), np.asarray(pbar, dtype=KC.NPT[ft])
    want, size = KC.grad_from_jvp(gq, pq, jv, jp)
    eps = np.finfo(KC.NPT[ft]).eps
    assert (np.abs(grad - want) <= min(KC.BOUND[ft], 8 * eps) * size).all(), np.max(np.abs(grad - want) / np.where(size > 0, size, 1))
    assert ((size == 0) <= (grad == 0)).all()
    # without cotangents at all: exact +0; each precipitation cotangent alone reaches the gradient
    zero = KC.host_vjp(host, ft, structs, ref["inv_dz"], ref["cols"], None, None, tables)[0]
    assert not zero.any() and not np.signbit(zero).any()
    for r in range(2):
        pb = [pq[0] if r == 0 else None, pq[1] if r == 1 else None]
        only = KC.host_vjp(host, ft, structs, ref["inv_dz"], ref["cols"], None, pb, tables)[0]
        mask = np.zeros_like(pq)
        mask[r] = pq[r]
        wantp, sizep = KC.grad_from_jvp(0 * gq, mask, jv, jp)
        assert (np.abs(only - wantp) <= 8 * eps * sizep).all() and only.any(), r


# ---- the NaN rule and the argument checks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_the_nan_rule(host, oracle, ft):
    """A NaN in a state input → every output of that point; in ρ or q_s → the flux of species s: the cell below and, from level 0, the precipitation outputs
    of rain and snow; in the gradient any of them, or a NaN cotangent, makes every grad[d] NaN.  No other point changes, bit for bit."""
    nm = no_exp(MAIN_CASE)[:5] + KC.SEDIMENTATION_ONLY
    ref, structs, tables, (cjv, cjp, ctend, cpr, _) = _call(host, ft, MAIN_CASE, "cold", "n2", nm=nm)
    n_col, n_lev = ref["n_col"], ref["n_lev"]
    args = (host, ft, structs, ref["inv_dz"])
    g, pbar = KC.cotangents(ref)
    i_top, i_bot = 5 * n_lev + 1, 5 * n_lev
    others = ~np.isin(np.arange(n_col * n_lev), (i_top, i_bot))
    for j in range(7):
        bad = [np.array(c) for c in ref["cols"]]
        bad[j][5, 1] = np.nan
        jv, jp, tend, pr, _ = KC.host_jvp(*args, bad, tables)
        assert np.isnan(jv[:, :, i_top]).all() and np.isnan(tend[:, i_top]).all(), j
        rows = [s for s in range(4) if j == 0 or j == 3 + s]                   # the species whose flux the NaN reaches
        for s in range(4):
            assert np.isnan(jv[:, s, i_bot]).all() == (s in rows) and np.isnan(tend[s, i_bot]) == (s in rows), (j, s)
        assert not np.isnan(jp[:, :, 5]).any() and not np.isnan(pr[:, 5]).any(), j      # level 1 is not the surface
        assert _same_bits(jv[:, :, others], cjv[:, :, others]) and _same_bits(tend[:, others], ctend[:, others]), j
        assert np.isnan(KC.host_vjp(*args, bad, g, pbar, tables)[0]).all(), j
        bad = [np.array(c) for c in ref["cols"]]
        bad[j][5, 0] = np.nan
        jv, jp, tend, pr, _ = KC.host_jvp(*args, bad, tables)
        for r in range(2):
            hit = j == 0 or j == 5 + r
            assert np.isnan(jp[r, :, 5]).all() == hit and np.isnan(pr[r, 5]) == hit, (j, r)
        assert _same_bits(np.delete(jp, 5, axis=2), np.delete(cjp, 5, axis=2)) and _same_bits(jv[:, :, i_top], cjv[:, :, i_top]), j
    gb = [np.array(a) for a in g]
    gb[2][i_bot] = np.nan
    assert np.isnan(KC.host_vjp(*args, ref["cols"], gb, pbar, tables)[0]).all()
    for r in range(2):
        pb = np.array(pbar)
        pb[r, 3] = np.nan
        assert np.isnan(KC.host_vjp(*args, ref["cols"], g, pb, tables)[0]).all()


def test_argument_checks(host, oracle):
    nm = no_exp(MAIN_CASE)[:3]
    ref, structs, tables, (jv, jp, _, _, rc) = _call(host, "f64", MAIN_CASE, "cold", "n3", nm=nm)
    args = (host, "f64", structs, ref["inv_dz"], ref["cols"])
    g, pbar = KC.cotangents(ref)
    flags = structs[0].flags
    obl, pro = _abi.CMX_1M_SED_SNOW_OBLATE, _abi.CMX_1M_SED_SNOW_PROLATE
    assert KC.host_jvp(*args, tables, override_flags=flags | obl | pro)[-1] == BAD
    for f in (flags | obl, flags | pro):
        assert KC.host_jvp(*args, tables, override_flags=f)[-1] == UNSUPPORTED and KC.host_vjp(*args, g, pbar, tables, override_flags=f)[-1] == UNSUPPORTED
    assert KC.host_jvp(*args, tables, ndir=0)[-1] == BAD and KC.host_jvp(*args, tables, ndir=_abi.CMX_PARAM_MAX_DIRS + 1)[-1] == BAD
    assert KC.host_jvp(*args, tables, use=(False, True, True, True, True))[-1] == BAD                  # d_mp is required
    # d_tps, d_stokes, d_chen_rain, d_chen_ice NULL: zero directions there, bit for bit
    quints = [P.column_parameter_direction_1m(structs[0], {"rain_drop_size_distribution_coefficient_n0": 2.0})] * 2
    t2 = KC.tables_of(quints)
    a = KC.host_jvp(*args, t2)
    b = KC.host_jvp(*args, t2, use=(True, False, False, False, False))
    assert b[-1] >= 0 and _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    ga = KC.host_vjp(*args, g, pbar, t2)[0]
    gb = KC.host_vjp(*args, g, pbar, t2, use=(True, False, False, False, False))[0]
    assert _same_bits(ga, gb)

    def copy():
        return [(type(t[0]) * 2)(*t) for t in t2]
    # a non-finite component anywhere in a direction
    for k, setter in ((0, lambda s: setattr(s.snow, "phi", float("inf"))), (1, lambda s: setattr(s, "cp_v", float("inf"))), (2, lambda s: setattr(s, "grav", float("nan"))),
                      (3, lambda s: s.a.__setitem__(1, float("nan"))), (4, lambda s: s.large_ice.H.__setitem__(2, float("inf")))):
        bad = copy()
        setter(bad[k][1])
        assert KC.host_jvp(*args, bad)[-1] == BAD, k
    # … comes before a direction on b or b_ρ, which is unsupported whatever the flags and the instantiation
    for case in (MAIN_CASE, ("default", True), ("alt", False)):
        s = KC.params("f64", case)
        for setter in (lambda r: setattr(r, "b_rho", 1e-3), lambda r: r.b.__setitem__(2, 1e-3)):
            bad = copy()
            setter(bad[3][1])
            assert KC.host_jvp(host, "f64", s, ref["inv_dz"], ref["cols"], bad)[-1] == UNSUPPORTED
            assert KC.host_vjp(host, "f64", s, ref["inv_dz"], ref["cols"], g, pbar, bad)[-1] == UNSUPPORTED
            bad[4][0].small_ice.A[0] = float("nan")
            assert KC.host_jvp(host, "f64", s, ref["inv_dz"], ref["cols"], bad)[-1] == BAD
    # the cutoff fields of the ice tables are not read: a direction there contributes nothing
    cut = copy()
    cut[4][0].small_ice.cutoff = cut[4][0].large_ice.cutoff = 1.0
    c = KC.host_jvp(*args, cut)
    assert _same_bits(a[0], c[0]) and _same_bits(a[1], c[1])
    # a direction on an exponent selects the run-time-flags instantiation for the whole call: other columns keep their VALUES to rounding, not their bits
    nm3 = nm[:2] + KC.EXPONENT_NAMES[:1]
    s, te = KC.directions("f64", MAIN_CASE, nm3)
    with_exp = KC.host_jvp(host, "f64", s, ref["inv_dz"], ref["cols"], te)
    without = KC.host_jvp(host, "f64", s, ref["inv_dz"], ref["cols"], te, ndir=2)
    assert with_exp[-1] == 0 and without[-1] == 1 and np.allclose(with_exp[0][:2], without[0][:2], rtol=1e-9, atol=0) and with_exp[0][2].any()
    # n_col = 0: CMX_OK, and the gradient entry writes zeros
    empty = [np.zeros((0, 3)) for _ in range(7)]
    assert KC.host_jvp(host, "f64", structs, ref["inv_dz"], empty, tables)[-1] == 0
    grad, _, _, rc = KC.host_vjp(host, "f64", structs, ref["inv_dz"], empty, None, None, tables)
    assert rc >= 0 and not grad.any()


# ---- the stand-alone program ------------------------------------------------------------------------------------------------------------------------
def test_the_stand_alone_program_runs(tmp_path):
    """tests/native/column_param_1m_host.cpp with its own main (the program to build with host sanitizer flags): compiled plainly here, run on the default
    parameter structs written as raw bytes; it checks the gradient against the sum over the jvp columns itself."""
    exe = tmp_path / "column_param_1m"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DCMX_COLUMN_PARAM_1M_MAIN", "-o", str(exe),
                    str(REPO / "tests" / "native" / "column_param_1m_host.cpp")], check=True)
    files = []
    for ft in ("f32", "f64"):
        mp, tps, stokes, cr, ci = KC.params(ft, MAIN_CASE)
        path = tmp_path / f"params_{ft}.bin"
        path.write_bytes(b"".join(bytes(memoryview(s)) for s in (mp.c, tps, stokes, cr, ci)))
        files.append(str(path))
    r = subprocess.run([str(exe), *files, str(mp.flags)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


def test_the_public_names_and_symbols():
    """The wrappers, their result tuples, the direction names and the four symbols of include/cmx.h §28."""
    import cmx
    from cmx import _lib
    assert cmx.ColumnParamJvp1M._fields == ("jvp", "jvp_precip_rai", "jvp_precip_sno", "tendencies", "precip_rai", "precip_sno")
    assert cmx.ColumnParamVjp1M._fields == ("grad", "tendencies", "precip_rai", "precip_sno", "wrt")
    assert callable(cmx.column_param_jvp_1m) and callable(cmx.column_param_vjp_1m)
    nm = P.COLUMN_1M_DIRECTION_NAMES
    assert set(P.MICROPHYSICS_1M_DIRECTION_NAMES) < set(nm) and len(set(nm)) == len(nm)
    for k in ("Chen2022_table_B1_q_coeff", "Chen2022_table_B1_a3_pow_coeff", "Chen2022_table_B1_ai[2]", "Chen2022_table_B1_ci[0]", "Chen2022_table_B3_Cs[3]",
              "Chen2022_table_B5_Al[1]", "Chen2022_table_B5_Hl[2]"):
        assert k in nm, k
    assert "Chen2022_table_B3_As[3]" not in nm and "Chen2022_ice_cutoff" not in nm
    for sfx in ("f32", "f64"):
        for product in ("jvp", "vjp"):
            assert getattr(_lib.lib(), f"cmx_mp1m_column_param_{product}_{sfx}").restype is C.c_int32
    mp = P.Microphysics1MParams("f64")
    d = P.column_parameter_direction_1m(mp, {"density_liquid_water": 2.0, "gravitational_acceleration": 0.5, "Chen2022_table_B5_Al[1]": 3.0,
                                             "Chen2022_table_B1_q_coeff": -1.0})
    assert d[0].cloud_liquid.rho_w == 2.0 and d[0].vel_rain.grav == 0.5 and d[2].rho_w == 2.0 and d[2].grav == 0.5 and d[4].large_ice.A[1] == 3.0
    assert d[3].rho_0 == -1.0 and d[1].R_v == 0.0
    for k in ("Chen2022_table_B1_bi[0]", "Chen2022_table_B1_b_rho_coeff"):
        with pytest.raises(ValueError, match="held fixed"):
            P.column_parameter_direction_1m(mp, {k: 1.0})
    with pytest.raises(ValueError):
        P.column_parameter_direction_1m(mp, {"Chen2022_ice_cutoff": 1.0})
