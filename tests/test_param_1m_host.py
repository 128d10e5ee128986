"""CPU tests of the parameter derivatives of the 1-moment tendencies (include/cmx.h §23), without a GPU: the host build of what the device entries run
(tests/native/param_derivatives_host.cpp on Mp1mJac) against central differences; tests/param_1m_cases.py has the parameters, the reference and the measure.
  * the constant tangents of make_mp1m_consts against central differences of the plain fold, every member and every name; value parts bit for bit;
  * `parameter_direction` for Microphysics1MParams against central differences of the Float64 struct constructor, every name, and the refactored constructor's
    one statement of the fields (`_values_1m`);
  * param_jvp_point in both float types, every case (default, alternative options, general exponents) on the cold, warm and limiter sets;
  * the value parts against the plain instantiation bit for bit, the instantiation choice, a column's bits against the directions per evaluation;
  * mutations of one parameter's column are rejected; the statuses of the device entries that return before any launch."""
import ctypes as C

import numpy as np
import pytest

import param_1m_cases as p1
import param_cases as pc
from cmx import _abi, _lib
from cmx import parameters as P
from jacobian_host_build import NPT, _arr, _same_bits, host_fixture, host_plain

host = host_fixture("param_derivatives_host")
derivatives = host_fixture("derivatives_host")


def host_param_jvp(host, ft, case, cols, nm, kp=0):
    """(S [4, P, n], tendencies [4, n], statuses) of host_mp1m_param_jvp in calls of at most CMX_PARAM_MAX_DIRS directions."""
    mp, tps = p1.params(ft, case)
    prs = p1.pairs(mp, case, nm)
    d_mp, d_tps = (type(mp.c) * len(nm))(*[a for a, _ in prs]), (type(tps) * len(nm))(*[b for _, b in prs])
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    n = x[0].size
    S = np.full((len(nm), 4, n), np.nan, dtype=NPT[ft])
    tend = np.full((4, n), np.nan, dtype=NPT[ft])
    fn = getattr(host, f"host_mp1m_param_jvp_{ft}")
    fn.restype = C.c_int32
    statuses = set()
    for p0 in range(0, len(nm), _abi.CMX_PARAM_MAX_DIRS):
        nd = min(_abi.CMX_PARAM_MAX_DIRS, len(nm) - p0)
        statuses.add(fn(C.byref(mp.c), C.byref(tps), C.c_uint32(mp.flags), C.c_int(kp), C.c_int64(n), _arr(ft, x), C.c_int32(nd), C.byref(d_mp[p0]),
                        C.byref(d_tps[p0]), _arr(ft, [S[p, o] for p in range(p0, p0 + nd) for o in range(4)]), _arr(ft, list(tend)) if p0 == 0 else None))
    return S.transpose(1, 0, 2), tend, statuses


def test_constant_tangents_match_central_differences_of_the_plain_fold(host):
    fn = host.host_mp1m_consts_f64
    fn.restype = C.c_int32

    def fold(case, ov, d_mp=None, d_tps=None):
        mp, tps = p1.params("f64", case, ov)
        out, val, tan = (np.empty(256) for _ in range(3))
        n = fn(C.byref(mp.c), C.byref(tps), C.c_uint32(mp.flags), C.byref(d_mp) if d_mp is not None else None, C.byref(d_tps) if d_tps is not None else None,
               out.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), tan.ctypes.data_as(C.c_void_p))
        assert 90 < n <= 256
        return out[:n], val[:n], tan[:n]
    for case in ("default", "exponents"):
        base = p1.overrides(case)
        mp, tps = p1.params("f64", case)
        live = 0
        for k, t in zip(p1.names(case), p1.theta(case)):
            d_mp, d_tps = P.parameter_direction(mp, {k: float(t)})
            out, val, tan = fold(case, base, d_mp, d_tps)
            assert _same_bits(out, val), k
            h = 1e-5 * abs(t)
            fd = (fold(case, {**base, k: t + h})[0] - fold(case, {**base, k: t - h})[0]) / ((t + h) - (t - h)) * t
            scale = np.maximum(np.abs(out), np.abs(fd))
            assert (np.abs(tan - fd) <= 1e-7 * scale).all(), (k, np.nonzero(np.abs(tan - fd) > 1e-7 * scale)[0], tan, fd)
            live += bool(tan.any())
        assert live >= 55, live


def test_parameter_direction_matches_central_differences_of_the_constructor():
    for case in ("default", "exponents"):
        base = p1.overrides(case)
        mp, tps = p1.params("f64", case)
        for k, t in zip(p1.names(case), p1.theta(case)):
            h = 1e-6 * abs(t)
            (mpp, tpp), (mpm, tpm) = p1.params("f64", case, {**base, k: t + h}), p1.params("f64", case, {**base, k: t - h})
            d_mp, d_tps = P.parameter_direction(mp, {k: 1.0})
            for got, plus, minus in ((d_mp, mpp.c, mpm.c), (d_tps, tpp, tpm)):
                fd = (np.frombuffer(bytes(plus)) - np.frombuffer(bytes(minus))) / ((t + h) - (t - h))
                g = np.frombuffer(bytes(got))
                assert (np.abs(g - fd) <= 1e-7 * np.maximum(np.abs(g), np.abs(fd))).all(), (k, g, fd)
            assert np.frombuffer(bytes(d_mp)).any() or np.frombuffer(bytes(d_tps)).any(), k
    mp = P.Microphysics1MParams("f64")
    row = P.microphysics_1m_direction_fields(mp, "snow_flake_length_scale")                  # one name, many fields: both r0, m0, a0, v0
    assert {"snow.mass.r0", "vel_snow.r0", "vel_rain.r0", "snow.mass.m0", "snow.area.a0", "vel_snow.v0"} <= set(row)
    assert len(P.MICROPHYSICS_1M_DIRECTION_NAMES) >= 59
    for bad in ("SB2006_collection_kernel_coeff_kcc", "not_a_parameter"):
        with pytest.raises(ValueError):
            P.parameter_direction(mp, {bad: 1.0})
    assert P.parameter_direction(P.Microphysics1MParams("f32"), {"temperature_water_freeze": 2.0})[1].T_freeze == 2.0


CASE_SETS = [(case, which) for case in p1.CASES for which in p1.SETS]


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("case,which", CASE_SETS)
def test_param_jvp_point_matches_the_oracle(host, derivatives, ft, case, which):
    cols = p1.reference(case, which)[0]
    nm = p1.names(case)
    S, tend, st = host_param_jvp(host, ft, case, cols, nm)
    assert st <= {0, 1}, st
    p1.assert_parity(ft, S, case, which, "host param_jvp 1m")
    # no exponent direction: the instantiation the tendencies entry selects, and its tendencies bit for bit
    mp, tps = p1.params(ft, case)
    rest = [k for k in nm if k not in p1.EXPONENT_NAMES and k != "snow_flake_length_scale"]
    S2, tend2, st2 = host_param_jvp(host, ft, case, cols, rest, kp=2)
    plain, rc = host_plain(derivatives, "mp1m", ft, (C.byref(mp.c), C.byref(tps), C.c_uint32(mp.flags)), cols)
    assert st2 == {rc} == {1 if case == "default" else 0}
    assert _same_bits(tend2, plain)
    if case != "default":      # the same instantiation in both calls: the columns do not depend on KP or on the other directions
        assert _same_bits(S[:, [nm.index(k) for k in rest]], S2) and _same_bits(tend, tend2)


def test_the_measure_rejects_a_wrong_column():
    cols, S_ref, kept, dead, _, resolved = p1.reference("default", "cold")
    nm = p1.names("default")
    sh = pc.shares(S_ref, kept)
    for p in np.nonzero(~dead)[0]:
        for f in (1.1, 0.0, -1.0):
            S = np.array(S_ref)
            S[:, p] *= f
            if sh[p] >= p1.LOW_SHARE:
                assert pc.row_error(S, S_ref)[:, p][:, kept].max() > p1.BOUND["f32"], (nm[p], f, sh[p])
            elif resolved[:, p].any():
                with pytest.raises(AssertionError):
                    p1.assert_low_share_columns(S, S_ref, kept, dead, resolved, nm, "mutation", report=False)


def test_statuses_before_any_launch():
    lib = _lib.lib()
    BAD, OK = _abi.CMX_ERR_BAD_ARG, _abi.CMX_OK
    for ft in ("f32", "f64"):
        mp, tps = P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft)
        d_mp, d_tps = P.parameter_direction(mp, {"rain_autoconversion_timescale": 1.0})
        jvp, vjp = getattr(lib, f"cmx_mp1m_param_jvp_{ft}"), getattr(lib, f"cmx_mp1m_param_vjp_{ft}")
        col = [C.c_void_p(4096)] * 7
        tab4, tab64 = (C.c_void_p * 4)(*[4096] * 4), (C.c_void_p * 64)(*[4096] * 64)
        w, t, dw, dt, fl = C.byref(mp.c), C.byref(tps), C.byref(d_mp), C.byref(d_tps), mp.flags
        assert jvp(None, t, fl, 8, *col, 1, dw, dt, tab64, None, None) == BAD
        assert jvp(w, t, fl, -1, *col, 1, dw, dt, tab64, None, None) == BAD
        assert jvp(w, t, fl, 16 * 0x7fffffff + 1, *col, 1, dw, dt, tab64, None, None) == _abi.CMX_ERR_UNSUPPORTED
        assert jvp(w, t, fl | (1 << 29), 0, *col, 1, dw, dt, tab64, None, None) != OK                 # the flags come before n = 0, as in the tendencies entry
        assert jvp(w, t, fl, 0, *([None] * 7), 0, None, None, None, None, None) == OK
        assert jvp(w, t, fl, 8, *([None] * 7), 1, dw, dt, tab64, None, None) == BAD
        for ndir in (0, -1, _abi.CMX_PARAM_MAX_DIRS + 1):
            assert jvp(w, t, fl, 8, *col, ndir, dw, dt, tab64, None, None) == BAD
        assert jvp(w, t, fl, 8, *col, 1, None, dt, tab64, None, None) == BAD
        assert jvp(w, t, fl, 8, *col, 1, dw, dt, None, None, None) == BAD
        dn = type(d_mp).from_buffer_copy(d_mp)
        dn.rain.n0 = float("nan")
        assert jvp(w, t, fl, 8, *col, 1, C.byref(dn), dt, tab64, None, None) == BAD
        g, ws = C.c_void_p(8192), C.c_void_p(16384)
        assert vjp(w, None, fl, 8, *col, tab4, 1, dw, dt, g, ws, None, None) == BAD
        assert vjp(w, t, fl, 0, *col, tab4, 0, dw, dt, g, ws, None, None) == BAD
        assert vjp(w, t, fl, 0, *col, tab4, 1, dw, dt, None, ws, None, None) == BAD
        assert vjp(w, t, fl, 8, *([None] * 7), tab4, 1, dw, dt, g, ws, None, None) == BAD
        assert vjp(w, t, fl, 8, *col, None, 1, dw, dt, g, ws, None, None) == BAD
        assert vjp(w, t, fl, 8, *col, tab4, 1, dw, dt, g, None, None, None) == BAD
        assert vjp(w, t, fl, 8, *col, tab4, 1, C.byref(dn), dt, g, ws, None, None) == BAD
