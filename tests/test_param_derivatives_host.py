"""CPU tests of the parameter derivatives of the SB2006 warm-rain tendencies (include/cmx.h §22), without a GPU: the host build of what the device entries run
(tests/native/param_derivatives_host.cpp — the fold of the constants with their tangents, csrc/cmx_param_tangent.hpp, and the point bodies param_jvp_point /
param_vjp_point of csrc/cmx_jacobian.hpp) against central differences; tests/param_cases.py has the parameters, the reference and the measure.
  * the constant tangents against central differences of the plain fold make_sb_consts<double>, every member and every name, and the value parts against the
    plain fold bit for bit;
  * `parameter_direction` against central differences of the Float64 struct constructors, every name;
  * param_jvp_point in both float types and both instantiations against the oracle's central differences, on the interior set and on the limiter set;
  * the value parts equal the plain instantiation bit for bit; a column's bits do not depend on the directions per evaluation;
  * mutations of one parameter's column (scaled by 1.1, zeroed, negated) are rejected by the measure;
  * the host mirror of the gradient reduction against a float64 sum of ḡ·(jvp columns) within the bound that holds for any order of summation;
  * the statuses of the device entries that return before any launch."""
import ctypes as C

import numpy as np
import pytest

import param_cases as pc
from cmx import _abi, _lib
from cmx import parameters as P
from jacobian_host_build import NPT, _arr, _same_bits, host_fixture, host_plain

host = host_fixture("param_derivatives_host")
derivatives = host_fixture("derivatives_host")


def _flat(struct):
    """The fields of a Float64 parameter struct."""
    return np.frombuffer(bytes(struct), dtype=np.float64)


def host_param_jvp(host, ft, limited, perturbed, cols, names=pc.NAMES, kp=0, with_tendencies=True):
    """(S [4, P, n], tendencies [4, n], statuses) of host_sb2006_param_jvp: direction p = θ_p along names[p], in calls of at most CMX_PARAM_MAX_DIRS directions
    (the tendencies are the first call's); statuses: the set of what the calls returned (1: the integer-exponent instantiation ran, 0: the general one)."""
    wr, tps, d_wr, d_tps = pc.directions(ft, limited, perturbed, names)
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    n = x[0].size
    S = np.full((len(names), 4, n), np.nan, dtype=NPT[ft])
    tend = np.full((4, n), np.nan, dtype=NPT[ft]) if with_tendencies else None
    fn = getattr(host, f"host_sb2006_param_jvp_{ft}")
    fn.restype = C.c_int32
    statuses = set()
    for p0 in range(0, len(names), _abi.CMX_PARAM_MAX_DIRS):
        nd = min(_abi.CMX_PARAM_MAX_DIRS, len(names) - p0)
        statuses.add(fn(C.byref(wr.c), C.byref(tps), C.c_uint32(_abi.CMX_SB2006_LIMITED if limited else 0), C.c_int(kp), C.c_int64(n), _arr(ft, x), C.c_int32(nd),
                        C.byref(d_wr[p0]), C.byref(d_tps[p0]), _arr(ft, [S[p, o] for p in range(p0, p0 + nd) for o in range(4)]),
                        _arr(ft, list(tend)) if tend is not None and p0 == 0 else None))
    return S.transpose(1, 0, 2), tend, statuses


def test_constant_tangents_match_central_differences_of_the_plain_fold(host):
    """Every member of SbConsts, every name: the tangent of the ParamTan fold along θ_p·∂/∂θ_p against (c(θ + h) − c(θ − h))/(θ⁺ − θ⁻)·θ_p of the plain fold
    with h = 1e-5·|θ_p|, within 1e-8 of the member's own size (a central difference of a smooth fold: truncation h² = 1e-10, rounding 2⁻⁵³/h = 1e-11); the
    value parts are the plain fold's bit for bit."""
    fn = host.host_sb2006_consts_f64
    fn.restype = C.c_int32

    def fold(ov, d_wr=None, d_tps=None):
        wr, tps = pc.params("f64", True, ov)
        out, val, tan = (np.empty(256) for _ in range(3))
        n = fn(C.byref(wr.c), C.byref(tps), C.byref(d_wr) if d_wr is not None else None, C.byref(d_tps) if d_tps is not None else None,
               out.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), tan.ctypes.data_as(C.c_void_p))
        assert 90 < n <= 256
        return out[:n], val[:n], tan[:n]
    for perturbed in (False, True):
        base = pc.overrides(perturbed)
        wr, tps = pc.params("f64", True, base)
        live = 0
        for k, t in zip(pc.NAMES, pc.theta(perturbed)):
            d_wr, d_tps = P.parameter_direction(wr, {k: float(t)})
            out, val, tan = fold(base, d_wr, d_tps)
            assert _same_bits(out, val), k
            h = 1e-5 * abs(t)
            fd = (fold({**base, k: t + h})[0] - fold({**base, k: t - h})[0]) / ((t + h) - (t - h)) * t
            # l2_gate_N and the limiters only feed compares and clamps, but their tangents are those of the fold all the same
            scale = np.maximum(np.abs(out), np.abs(fd))
            assert (np.abs(tan - fd) <= 1e-8 * scale).all(), (k, np.nonzero(np.abs(tan - fd) > 1e-8 * scale)[0], tan, fd)
            live += bool(tan.any())
        assert live >= 30, live


def test_parameter_direction_matches_central_differences_of_the_constructors():
    """Every name of the table: the direction structs against central differences of the Float64 struct constructors (h = 1e-6·|θ|, bound 1e-8 of the field's
    derivative scale), for the default and the perturbed dictionary; names that reach no field raise ValueError."""
    for perturbed in (False, True):
        base = pc.overrides(perturbed)
        wr, tps = pc.params("f64", True, base)
        for k in P.WARM_RAIN_2M_DIRECTION_FIELDS:
            t = base.get(k, P.DEFAULT_PARAMETERS[k])
            h = 1e-6 * abs(t)
            (wp, tp), (wm, tm) = pc.params("f64", True, {**base, k: t + h}), pc.params("f64", True, {**base, k: t - h})
            d_wr, d_tps = P.parameter_direction(wr, {k: 1.0})
            for got, plus, minus in ((d_wr, wp.c, wm.c), (d_tps, tp, tm)):
                fd = (_flat(plus) - _flat(minus)) / ((t + h) - (t - h))
                g = _flat(got)
                assert (np.abs(g - fd) <= 1e-8 * np.maximum(np.abs(g), np.abs(fd))).all(), (k, g, fd)
            assert _flat(d_wr).any() or _flat(d_tps).any(), k
    wr = P.WarmRainParams2M("f64")
    d2 = P.parameter_direction(wr, {"SB2006_raindrops_min_mass": 2.0})[0].seifert_beheng
    assert d2.pdf_r.xr_min == d2.pdf_c.xc_max == d2.acnv.x_star == 2.0               # one name, three fields
    for bad in ("SB2006_raindrops_terminal_velocity_coeff_aR", "not_a_parameter", "snow_flake_size_distribution_coefficient_mu"):
        with pytest.raises(ValueError):
            P.parameter_direction(wr, {bad: 1.0})
    assert P.parameter_direction(P.Microphysics2MParams("f32"), {"gas_constant_vapor": 3.0})[1].R_v == 3.0


CASES = [(limited, perturbed, which) for which in ("interior", "limiters") for limited in (True, False) for perturbed in (False, True)]


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("limited,perturbed,which", CASES)
def test_param_jvp_point_matches_the_oracle(host, derivatives, ft, limited, perturbed, which):
    cols = pc.reference(limited, perturbed, which)[0]
    S, tend, st = host_param_jvp(host, ft, limited, perturbed, cols)
    assert st <= {0, 1}, st                 # every call ran (a call with an exponent direction: the general instantiation)
    pc.assert_parity(ft, S, limited, perturbed, which, "host param_jvp")
    # the value parts: the plain instantiation of the general form
    wr, tps = pc.params(ft, limited, pc.overrides(perturbed))
    head = (C.byref(wr.c), C.byref(tps), C.c_uint32(_abi.CMX_SB2006_LIMITED if limited else 0))
    names = [k for k in pc.NAMES if k not in pc.EXPONENTS]
    S2, tend2, st2 = host_param_jvp(host, ft, limited, perturbed, cols, names=names, kp=2)
    plain, rc = host_plain(derivatives, "sb2006", ft, head, cols)
    assert st2 == {rc} == {0 if perturbed else 1}        # no exponent direction: the instantiation the tendencies entry selects
    assert _same_bits(tend2, plain)
    if perturbed:                                         # the same instantiation in both calls: the columns do not depend on KP or on the other directions
        keep = [pc.NAMES.index(k) for k in names]
        assert _same_bits(S[:, keep], S2) and _same_bits(tend, tend2)


def test_directions_per_evaluation_do_not_change_a_column(host):
    cols = [c[:257] for c in pc.states("interior")]
    for ft in ("f32", "f64"):
        names = pc.NAMES[:7]
        ref = host_param_jvp(host, ft, True, False, cols, names=names, kp=1)[0]
        for kp in (2, 4):
            assert _same_bits(ref, host_param_jvp(host, ft, True, False, cols, names=names, kp=kp)[0]), (ft, kp)
        for p in (0, 3, 6):                                # alone
            assert _same_bits(ref[:, p:p + 1], host_param_jvp(host, ft, True, False, cols, names=names[p:p + 1], kp=4)[0]), (ft, p)


def test_the_measure_rejects_a_wrong_column():
    """One parameter's column scaled by 1.1, zeroed or negated — for every live parameter that reaches LOW_SHARE of a row, the row measure must reject it at the
    Float32 bound already; the low-share ones are rejected by the column-scale assertion."""
    cols, S_ref, kept, dead, _ = pc.reference(True, False, "interior")
    sh = pc.shares(S_ref, kept)
    for p in np.nonzero(~dead)[0]:
        for f in (1.1, 0.0, -1.0):
            S = np.array(S_ref)
            S[:, p] *= f
            e = pc.row_error(S, S_ref)[:, p][:, kept].max()
            if sh[p] >= pc.LOW_SHARE:
                assert e > pc.BOUND["f32"], (pc.NAMES[p], f, e, sh[p])
            else:
                with pytest.raises(AssertionError):
                    pc.assert_low_share_columns(S, S_ref, kept, dead, "mutation", report=False)


def test_host_gradient_reduction_matches_the_sum_of_columns(host):
    rng = np.random.default_rng(5)
    names = pc.NAMES[12:16]
    for ft in ("f32", "f64"):
        for n in (1, 65, 1025):
            cols = [np.ascontiguousarray(c[:n], dtype=NPT[ft]) for c in pc.states("interior")]
            S = host_param_jvp(host, ft, True, True, cols, names=names)[0]
            cot = [rng.standard_normal(n).astype(NPT[ft]), None, rng.standard_normal(n).astype(NPT[ft]), rng.standard_normal(n).astype(NPT[ft])]
            wr, tps, d_wr, d_tps = pc.directions(ft, True, True, names)
            grad = np.full(len(names), np.nan)
            fn = getattr(host, f"host_sb2006_param_vjp_{ft}")
            fn.restype = C.c_int32
            st = fn(C.byref(wr.c), C.byref(tps), C.c_uint32(1), C.c_int64(n), _arr(ft, cols), _arr(ft, cot), C.c_int32(len(names)), d_wr, d_tps,
                    grad.ctypes.data_as(C.c_void_p), None)
            assert st == 0
            terms = sum(g.astype(np.float64)[None] * S[o].astype(np.float64) for o, g in enumerate(cot) if g is not None)      # [P, n]
            # per point the device forms Σ_o in the float type (fma chain): each term within 4 roundings of the float type of Σ_o |ḡ_o S_o|
            absum = sum(np.abs(g.astype(np.float64)[None] * S[o].astype(np.float64)) for o, g in enumerate(cot) if g is not None)
            tol = 2 * n * 2.0 ** -53 * np.abs(terms).sum(axis=1) + 4 * np.finfo(NPT[ft]).eps * absum.sum(axis=1)
            assert (np.abs(grad - terms.sum(axis=1)) <= tol).all(), (ft, n, grad, terms.sum(axis=1), tol)


def test_statuses_before_any_launch():
    lib = _lib.lib()
    BAD, OK = _abi.CMX_ERR_BAD_ARG, _abi.CMX_OK
    for ft in ("f32", "f64"):
        wr, tps = P.WarmRainParams2M(ft), P.ThermodynamicsParameters(ft)
        d_wr, d_tps = P.parameter_direction(wr, {"SB2006_collection_kernel_coeff_kcc": 1.0})
        jvp, vjp = getattr(lib, f"cmx_sb2006_warm_rain_param_jvp_{ft}"), getattr(lib, f"cmx_sb2006_warm_rain_param_vjp_{ft}")
        col = [C.c_void_p(4096)] * 7
        tab4, tab64 = (C.c_void_p * 4)(*[4096] * 4), (C.c_void_p * 64)(*[4096] * 64)
        w, t, dw, dt = C.byref(wr.c), C.byref(tps), C.byref(d_wr), C.byref(d_tps)
        assert jvp(None, t, 1, 8, *col, 1, dw, dt, tab64, None, None) == BAD
        assert jvp(w, t, 1, -1, *col, 1, dw, dt, tab64, None, None) == BAD
        assert jvp(w, t, 1, 16 * 0x7fffffff + 1, *col, 1, dw, dt, tab64, None, None) == _abi.CMX_ERR_UNSUPPORTED
        assert jvp(w, t, 1, 0, *([None] * 7), 0, None, None, None, None, None) == OK                 # n = 0 returns first
        assert jvp(w, t, 1, 8, *([None] * 7), 1, dw, dt, tab64, None, None) == BAD                   # NULL columns
        for ndir in (0, -1, _abi.CMX_PARAM_MAX_DIRS + 1):
            assert jvp(w, t, 1, 8, *col, ndir, dw, dt, tab64, None, None) == BAD
        assert jvp(w, t, 1, 8, *col, 1, None, dt, tab64, None, None) == BAD                          # NULL direction table
        assert jvp(w, t, 1, 8, *col, 1, dw, dt, None, None, None) == BAD                             # no output at all
        assert jvp(w, t, 1, 8, *col, 1, dw, dt, (C.c_void_p * 4)(), (C.c_void_p * 4)(), None) == BAD
        assert jvp(w, t, 2, 8, *col, 1, dw, dt, tab64, None, None) == BAD                            # unknown flag
        for bad_value in (float("nan"), float("inf")):
            dn = type(d_wr).from_buffer_copy(d_wr)
            dn.seifert_beheng.accr.kcr = bad_value
            assert jvp(w, t, 1, 8, *col, 1, C.byref(dn), dt, tab64, None, None) == BAD               # a non-finite component
            tn = type(d_tps).from_buffer_copy(d_tps)
            tn.cp_l = bad_value
            assert jvp(w, t, 1, 8, *col, 1, dw, C.byref(tn), tab64, None, None) == BAD
        bad = P.WarmRainParams2M(ft)
        bad.c.seifert_beheng.pdf_r.lambda_min, bad.c.seifert_beheng.pdf_r.lambda_max = 1e4, 1e3
        assert jvp(C.byref(bad.c), t, 1, 8, *col, 1, dw, dt, tab64, None, None) == BAD               # unordered limiters
        g, ws = C.c_void_p(8192), C.c_void_p(16384)
        assert vjp(w, None, 1, 8, *col, tab4, 1, dw, dt, g, ws, None, None) == BAD
        assert vjp(w, t, 1, -1, *col, tab4, 1, dw, dt, g, ws, None, None) == BAD
        # n = 0 sets grad: every check but the columns applies (the one valid call would enqueue a memset and is made on the device only)
        assert vjp(w, t, 1, 0, *col, tab4, 0, dw, dt, g, ws, None, None) == BAD
        assert vjp(w, t, 1, 0, *col, tab4, 1, dw, dt, None, ws, None, None) == BAD
        assert vjp(w, t, 1, 0, *col, tab4, 1, dw, dt, g, None, None, None) == BAD
        assert vjp(w, t, 1, 0, *([None] * 7), tab4, 1, None, dt, g, ws, None, None) == BAD
        assert vjp(w, t, 1, 0, *([None] * 7), None, 1, dw, dt, g, ws, None, None) == BAD
        assert vjp(w, t, 4, 0, *([None] * 7), tab4, 1, dw, dt, g, ws, None, None) == BAD              # unknown flag
        dn = type(d_wr).from_buffer_copy(d_wr)
        dn.condevap_tau_relax = float("nan")
        assert vjp(w, t, 1, 0, *([None] * 7), tab4, 1, C.byref(dn), dt, g, ws, None, None) == BAD      # a non-finite direction
        assert vjp(C.byref(bad.c), t, 1, 0, *([None] * 7), tab4, 1, dw, dt, g, ws, None, None) == BAD  # unordered limiters
        assert vjp(w, t, 1, 8, *([None] * 7), tab4, 1, dw, dt, g, ws, None, None) == BAD
        assert vjp(w, t, 1, 8, *col, tab4, 17, dw, dt, g, ws, None, None) == BAD
        assert vjp(w, t, 1, 8, *col, None, 1, dw, dt, g, ws, None, None) == BAD                      # NULL cotangent table
        assert vjp(w, t, 1, 8, *col, tab4, 1, None, dt, g, ws, None, None) == BAD
        assert vjp(w, t, 1, 8, *col, tab4, 1, dw, dt, None, ws, None, None) == BAD                   # NULL grad
        assert vjp(w, t, 1, 8, *col, tab4, 1, dw, dt, g, None, None, None) == BAD                    # NULL workspace
        assert vjp(w, t, 4, 8, *col, tab4, 1, dw, dt, g, ws, None, None) == BAD
