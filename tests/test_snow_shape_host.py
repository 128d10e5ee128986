"""Snow shapes of the Chen-2022 snow fall speed, CPU side (CM1.terminal_velocity(snow, Ch2022.large_ice, ρ, q, CM1.Oblate() | CM1.Prolate()),
src/Microphysics1M.jl:155-195, 299-324):

  * the float64 restatement tests/snow_shape_ref.py, pinned four ways (B4 coefficients, the unshaped known answer, the oracle's unshaped snow
    speed, the reference's qualitative shape checks);
  * the device point function and its host folding (csrc/cmx_mp1m_vel.hpp vel_snow_shaped, make_snow_shape_consts) compiled by g++
    (tests/native/snow_shape_host.cpp) against the restatement;
  * the argument checks of the C ABI and of the Python API that need no GPU, and the Julia binding's use of the CM1 shape types."""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import snow_shape_ref as R
from cmx import _abi, _lib
from cmx import parameters as P

REPO = Path(__file__).resolve().parent.parent
KATS = json.loads((REPO / "tests" / "golden" / "snow_shape_kats.json").read_text())
MP1M_KATS = json.loads((REPO / "tests" / "golden" / "mp1m_kats.json").read_text())
NPT = {"f32": np.float32, "f64": np.float64}
CT = {"f32": C.c_float, "f64": C.c_double}
SHAPES = {"aspr": (None, _abi.CMX_SNOW_SHAPE_ASPR), "oblate": (R.Oblate(), _abi.CMX_SNOW_SHAPE_OBLATE),
          "prolate": (R.Prolate(), _abi.CMX_SNOW_SHAPE_PROLATE)}


def _params(ft):
    return P.Microphysics1MParams(ft).c, P.Chen2022VelTypeIce(ft)


def random_states(n, seed):
    """ρ ∈ [0.3, 1.4], q log-uniform in [1e-10, 1e-2], plus exact zeros, negatives and ϵ-neighbourhood values of q."""
    g = np.random.default_rng(seed)
    rho = g.uniform(0.3, 1.4, n)
    q = 10.0 ** g.uniform(-10, -2, n)
    k = n // 50
    q[:k] = 0.0
    q[k:2 * k] = -q[k:2 * k]
    rho[2 * k:2 * k + k // 4] = 0.0            # ρ = 0 (outside the domain)
    rho[2 * k + k // 4:2 * k + k // 2] = -0.5
    return rho, q


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def test_restatement_reproduces_the_B4_large_ice_coefficients():
    k = KATS["chen2022_large_ice_B4"]
    mp, ci = _params("f64")
    aiu, bi, ciu = R.large_ice_coeffs(ci.large_ice, k["rho"], float(mp.snow.rho_i))
    tol = k["rtol_eps"] * np.finfo(np.float64).eps
    np.testing.assert_allclose(np.array(aiu, dtype=np.float64), k["aiu"], rtol=tol, atol=0)
    np.testing.assert_allclose(bi, k["bi"], rtol=tol, atol=0)
    np.testing.assert_allclose(ciu, k["ciu"], rtol=tol, atol=0)


def test_restatement_reproduces_the_unshaped_known_answer():
    k = MP1M_KATS["chen2022_sedimentation_velocities"]["extra"]["snow"]
    mp, ci = _params("f64")
    w = float(R.snow_velocity(mp, ci, k["rho"], k["q_sno"]))
    assert w == pytest.approx(k["w_sno"], rel=1e-12)


def test_restatement_matches_the_oracle_unshaped_snow_speed():
    import oracle_binding as ob
    mp, ci = _params("f64")
    rho, q = random_states(20_000, 11)
    keep = rho > 0
    rho, q = rho[keep], q[keep]
    z = np.zeros_like(rho)
    ref = ob.sedimentation_velocities(_abi.F64, mp, P.StokesRegimeVelType("f64"), P.Chen2022VelTypeRain("f64"), ci, rho, z, z, z, q,
                                      float32_gates=False)["w_sno"]
    got = R.snow_velocity(mp, ci, rho, q)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


def test_restatement_passes_the_reference_shape_checks():
    k = KATS["snow_shape_checks"]
    mp, ci = _params("f64")
    w = {nm: float(R.snow_velocity(mp, ci, k["rho"], k["q_sno"], sh)) for nm, sh in (("oblate", R.Oblate()), ("prolate", R.Prolate()))}
    for nm, sh in (("oblate", R.Oblate()), ("prolate", R.Prolate())):
        assert w[nm] > 0
        assert float(R.snow_velocity(mp, ci, k["rho"], 0.0, sh)) == pytest.approx(0, abs=np.finfo(np.float64).eps)
        assert float(R.snow_velocity(mp, ci, k["rho"], k["q_sno"] * k["q_factor_bigger"], sh)) > w[nm]
    assert 0.1 < w["oblate"] / w["prolate"] < 10


# ---- the point function and its host folding ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    out = REPO / "tests" / "native" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libsnow_shape_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so),
                    str(REPO / "tests" / "native" / "snow_shape_host.cpp")], check=True)
    return C.CDLL(str(so))


def _host_call(host, ft, shape, rho, q):
    mp, ci = _params(ft)
    x = [np.ascontiguousarray(a, dtype=NPT[ft]) for a in (rho, q)]
    w = np.empty_like(x[0])
    fn = getattr(host, f"snow_velocity_{ft}")
    fn.restype = C.c_int32
    P_ = C.POINTER(CT[ft])
    rc = fn(C.byref(mp), C.byref(ci), C.c_uint32(shape), C.c_int64(w.size), x[0].ctypes.data_as(P_), x[1].ctypes.data_as(P_), w.ctypes.data_as(P_))
    return rc, x, w


@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_point_function_matches_the_restatement(host, ft, shape):
    sh, code = SHAPES[shape]
    rho, q = random_states(100_000, 7)
    rc, (r, qq), w = _host_call(host, ft, code, rho, q)
    assert rc == _abi.CMX_OK
    mp64, ci64 = _params("f64")
    ref = R.snow_velocity(mp64, ci64, r.astype(np.float64), qq.astype(np.float64), sh, ft=ft)
    bad = (r <= 0) if ft == "f64" else np.zeros(r.shape, bool)     # Float64: ρ ≤ 0 gives NaN (include/cmx.h)
    assert np.isnan(w[bad]).all()
    ok = ~bad & (r > 0)
    rtol = {"f32": 1e-3, "f64": 1e-6}[ft]
    floor = {"f32": 1e-30, "f64": 1e-290}[ft]
    err = np.abs(w[ok].astype(np.float64) - ref[ok]) / np.maximum(np.abs(ref[ok]), floor)
    assert np.isfinite(w[ok]).all()
    assert err.max() <= rtol, (shape, ft, float(err.max()), int(np.argmax(err)))
    absent = ok & (qq <= R.EPS_NUMERICS[ft])
    assert (w[absent] == 0).all()                                # q ≤ ϵ: exactly 0
    assert (w >= 0)[~np.isnan(w)].all()


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_point_function_nan_inputs_give_nan(host, ft):
    rho = np.array([np.nan, 1.0, np.nan, -np.nan, 1.0])
    q = np.array([1e-4, np.nan, np.nan, 1e-4, -np.nan])
    for code in (0, 1, 2):
        rc, _, w = _host_call(host, ft, code, rho, q)
        assert rc == _abi.CMX_OK and np.isnan(w).all()


def test_point_function_shapes_differ_from_the_fixed_aspect_ratio(host):
    """The shape is not silently ignored: at the reference's state the three methods give three different speeds, in the restatement's ratios."""
    k = KATS["snow_shape_checks"]
    w = {nm: float(_host_call(host, "f64", code, [k["rho"]], [k["q_sno"]])[2][0]) for nm, (_, code) in SHAPES.items()}
    mp, ci = _params("f64")
    for nm, (sh, _) in SHAPES.items():
        assert w[nm] == pytest.approx(float(R.snow_velocity(mp, ci, k["rho"], k["q_sno"], sh)), rel=1e-9)
    assert len({round(v, 6) for v in w.values()}) == 3


# ---- argument checks without a GPU -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_c_entry_refuses_bad_arguments(ft):
    lib = _lib.lib()
    fn = getattr(lib, f"cmx_snow_terminal_velocity_{ft}")
    mp, ci = _params(ft)
    col = (CT[ft] * 4)()
    p = C.cast(col, C.c_void_p)
    assert fn(C.byref(mp), C.byref(ci), 3, 4, p, p, p, None) == _abi.CMX_ERR_BAD_ARG            # snow_shape > 2
    assert fn(C.byref(mp), C.byref(ci), 0xffffffff, 4, p, p, p, None) == _abi.CMX_ERR_BAD_ARG
    assert fn(None, C.byref(ci), 1, 4, p, p, p, None) == _abi.CMX_ERR_BAD_ARG
    assert fn(C.byref(mp), None, 1, 4, p, p, p, None) == _abi.CMX_ERR_BAD_ARG
    assert fn(C.byref(mp), C.byref(ci), 1, -1, p, p, p, None) == _abi.CMX_ERR_BAD_ARG
    assert fn(C.byref(mp), C.byref(ci), 1, 4, None, p, p, None) == _abi.CMX_ERR_BAD_ARG
    assert fn(C.byref(mp), C.byref(ci), 2, 4, p, p, None, None) == _abi.CMX_ERR_BAD_ARG
    assert fn(C.byref(mp), C.byref(ci), 2, 0, None, None, None, None) == _abi.CMX_OK                # nothing to do, nothing launched
    assert fn(C.byref(mp), C.byref(ci), 2, 16 * 0x7fffffff + 1, p, p, p, None) == _abi.CMX_ERR_UNSUPPORTED


def test_only_the_column_entry_takes_the_shape_bits():
    lib = _lib.lib()
    mp, tps = P.Microphysics1MParams("f32"), P.ThermodynamicsParameters("f32")
    st, cr, ci = P.StokesRegimeVelType("f32"), P.Chen2022VelTypeRain("f32"), P.Chen2022VelTypeIce("f32")
    both = _abi.CMX_1M_SED_SNOW_OBLATE | _abi.CMX_1M_SED_SNOW_PROLATE
    col = (C.c_float * 4)()
    p = C.cast(col, C.c_void_p)
    cols7, cols4 = (C.c_void_p * 7)(*[p.value] * 7), (C.c_void_p * 4)(*[p.value] * 4)
    f = lib.cmx_mp1m_column_tendencies_sedimentation_f32
    assert f(C.byref(mp.c), C.byref(tps), C.byref(st), C.byref(cr), C.byref(ci), mp.flags | both, 0.0, 0.0, 0, 1, 4, p, cols7, cols4, None, None,
             None) == _abi.CMX_ERR_BAD_ARG
    for bit in (_abi.CMX_1M_SED_SNOW_OBLATE, _abi.CMX_1M_SED_SNOW_PROLATE):          # a shape bit does not hide an invalid option set
        bad = mp.flags | _abi.CMX_1M_RAIN_ACNV_PRESCRIBED_ND | _abi.CMX_1M_RAIN_ACNV_KESSLER | bit
        assert f(C.byref(mp.c), C.byref(tps), C.byref(st), C.byref(cr), C.byref(ci), bad, 0.0, 0.0, 0, 1, 4, p, cols7, cols4, None, None,
                 None) == _abi.CMX_ERR_BAD_ARG
        # n_col = 0: a valid call that launches nothing — the bit is accepted here
        assert f(C.byref(mp.c), C.byref(tps), C.byref(st), C.byref(cr), C.byref(ci), mp.flags | bit, 0.0, 0.0, 0, 0, 4, p, cols7, cols4, None, None,
                 None) == _abi.CMX_OK
        # … and refused by every other 1-moment entry, as before
        assert lib.cmx_mp1m_tendencies_f32(C.byref(mp.c), C.byref(tps), mp.flags | bit, 0, *[None] * 11, None) == _abi.CMX_ERR_BAD_ARG


def test_python_entry_refuses_bad_arguments():
    import cmx
    mp, ci = P.Microphysics1MParams("f32"), P.Chen2022VelTypeIce("f32")
    x = torch.zeros(8)
    with pytest.raises(TypeError, match="snow_shape"):
        cmx.snow_terminal_velocity(mp, ci, x, x, "oblate")
    with pytest.raises(TypeError, match="snow_shape"):
        cmx.snow_terminal_velocity(mp, ci, x, x, cmx.AbstractSnowShape())
    with pytest.raises(TypeError, match="Microphysics1MParams"):
        cmx.snow_terminal_velocity(P.Microphysics2MParams("f32"), ci, x, x, cmx.Oblate())
    with pytest.raises(ValueError, match="resident on the GPU"):            # no CPU path
        cmx.snow_terminal_velocity(mp, ci, x, x, cmx.Oblate())
    tps = P.ThermodynamicsParameters("f32")
    cols = [torch.zeros(2, 4) for _ in range(7)]
    with pytest.raises(TypeError, match="snow_shape"):
        cmx.column_tendencies_sedimentation_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), mp, tps, P.StokesRegimeVelType("f32"),
                                               P.Chen2022VelTypeRain("f32"), ci, torch.ones(4), *cols, snow_shape=1)
    assert issubclass(cmx.Oblate, cmx.AbstractSnowShape) and issubclass(cmx.Prolate, cmx.AbstractSnowShape)


def test_julia_binding_uses_only_the_cm1_names_of_the_fixture():
    """tools/check_julia_shim.py checks the CMP / BMT / AM / AA / QUAD names of julia/CMXExt.jl, not CM1: every `CM1.<name>` the binding uses must be one
    of the CM1 types listed (with their file:line) in tests/golden/snow_shape_kats.json."""
    import sys
    sys.path.insert(0, str(REPO / "tools"))
    import check_julia_shim as chk
    shim = chk.strip_julia((REPO / "julia" / "CMXExt.jl").read_text())
    used = set(re.findall(r"\bCM1\.([^\W\d][\w!]*)", shim))
    names = KATS["snow_shape_types"]["names"]
    assert used, "the binding does not use the CM1 snow shapes"
    assert used <= set(names), sorted(used - set(names))
    assert {"Oblate", "Prolate", "AbstractSnowShape"} <= used
    assert re.search(r"^import CloudMicrophysics\.Microphysics1M as CM1$", (REPO / "julia" / "CMXExt.jl").read_text(), flags=re.M)
