"""Snow shapes of the Chen-2022 snow fall speed on the device (-m gpu), through the C ABI (cmx_snow_terminal_velocity_*) and the 1-moment column
step with a CMX_1M_SED_SNOW_* bit; the float64 reference is the NumPy restatement tests/snow_shape_ref.py (pinned in tests/test_snow_shape_host.py).
CM1.terminal_velocity(snow, Ch2022.large_ice, ρ, q, CM1.Oblate() | CM1.Prolate()) — src/Microphysics1M.jl:155-195, 299-324."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import parity
import snow_shape_ref as R
from cmx import _abi
from cmx import parameters as P
from test_mp1m_column import _oracle
from test_snow_shape_host import random_states

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
KATS = json.loads((REPO / "tests" / "golden" / "snow_shape_kats.json").read_text())
DT = {"f32": torch.float32, "f64": torch.float64}
SHAPES = {"aspr": None, "oblate": "Oblate", "prolate": "Prolate"}
COL_NAMES = ("dq_lcl_dt", "dq_icl_dt", "dq_rai_dt", "dq_sno_dt")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _shape(nm):
    import cmx
    return getattr(cmx, SHAPES[nm])() if SHAPES[nm] else None


def _ref_shape(nm):
    return getattr(R, SHAPES[nm])() if SHAPES[nm] else None


def _bits(t):
    """the bit patterns (Float64: ρ ≤ 0 gives NaN, which torch.equal never calls equal)"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _w(ft, rho, q, nm):
    import cmx
    return cmx.snow_terminal_velocity(P.Microphysics1MParams(ft), P.Chen2022VelTypeIce(ft), rho, q, _shape(nm))


@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("nm", list(SHAPES))
def test_every_point_inside_the_plain_bound(dev, ft, nm):
    n = 1_000_003
    rho, q = random_states(n, 21)
    keep = rho > 0
    rho, q = rho[keep], q[keep]
    r_t, q_t = torch.tensor(rho, dtype=DT[ft], device=dev), torch.tensor(q, dtype=DT[ft], device=dev)
    got = _w(ft, r_t, q_t, nm).cpu().numpy().astype(np.float64)
    mp64, ci64 = P.Microphysics1MParams("f64").c, P.Chen2022VelTypeIce("f64")
    ref = R.snow_velocity(mp64, ci64, r_t.cpu().numpy().astype(np.float64), q_t.cpu().numpy().astype(np.float64), _ref_shape(nm), ft=ft)
    rep = parity.assert_parity({"w_sno": got}, {"w_sno": ref}, parity.RTOL[ft], names=("w_sno",), what=f"snow fall speed {nm} {ft}",
                               family="1-moment (a2)", pinned_by="tests/snow_shape_ref.py (pinned by the B4 / unshaped KATs and the oracle)")
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), parity.FLOOR[ft])
    assert rel.max() <= parity.RTOL[ft], (nm, ft, float(rel.max()), int(np.argmax(rel)))
    assert (got[q <= R.EPS_NUMERICS[ft]] == 0).all()
    print(f"\n[snow shape parity] {nm} {ft}: {rep}, worst plain relative error {rel.max():.3e}")


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_aspr_is_bit_identical_to_the_sedimentation_w_sno(dev, ft):
    import cmx
    rho, q = random_states(300_007, 5)
    r_t, q_t = torch.tensor(rho, dtype=DT[ft], device=dev), torch.tensor(q, dtype=DT[ft], device=dev)
    idx = torch.arange(3, r_t.numel(), 101, device=dev)
    r_t[idx] = float("nan")
    q_t[idx + 1] = float("nan")
    nan = torch.zeros_like(r_t, dtype=torch.bool)
    nan[idx] = True
    nan[idx + 1] = True
    mp = P.Microphysics1MParams(ft)
    sed = cmx.sedimentation_velocities(mp, P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft), P.Chen2022VelTypeIce(ft), r_t, None, None, None, q_t).w_sno
    w = _w(ft, r_t, q_t, "aspr")
    torch.cuda.synchronize()
    # every point without a NaN input, ρ ≤ 0 included (Float64: NaN in both), bit for bit
    assert torch.equal(_bits(w[~nan]), _bits(sed[~nan]))
    assert bool(torch.isnan(w[nan]).all())                      # the NaN rule of include/cmx.h
    if ft == "f64":
        assert bool(torch.isnan(w[r_t <= 0]).all())


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_reference_shape_checks_on_the_device(dev, ft):
    k = KATS["snow_shape_checks"]
    x = lambda v: (torch.tensor([k["rho"]], dtype=DT[ft], device=dev), torch.tensor([v], dtype=DT[ft], device=dev))  # noqa: E731
    w = {nm: float(_w(ft, *x(k["q_sno"]), nm)[0]) for nm in ("oblate", "prolate")}
    for nm in ("oblate", "prolate"):
        assert w[nm] > 0
        assert abs(float(_w(ft, *x(0.0), nm)[0])) <= torch.finfo(DT[ft]).eps
        assert float(_w(ft, *x(k["q_sno"] * k["q_factor_bigger"]), nm)[0]) > w[nm]
    assert 0.1 < w["oblate"] / w["prolate"] < 10


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_ragged_sizes_and_offset_views_are_bit_identical(dev, ft):
    rho, q = random_states(40_000, 9)
    r_t, q_t = torch.tensor(rho, dtype=DT[ft], device=dev), torch.tensor(q, dtype=DT[ft], device=dev)
    full = _w(ft, r_t, q_t, "oblate")
    for lo, hi in ((0, 1), (0, 3), (1, 2), (1, 40_000), (3, 39_997), (2, 1027), (0, 39_999), (5, 6)):
        assert torch.equal(_bits(_w(ft, r_t[lo:hi], q_t[lo:hi], "oblate")), _bits(full[lo:hi])), (lo, hi)
    # misaligned output, aligned inputs: the one-point-per-lane path for everything
    out = torch.empty(40_001, dtype=DT[ft], device=dev)
    import ctypes as C
    from cmx import _lib
    fn = getattr(_lib.lib(), f"cmx_snow_terminal_velocity_{ft}")
    mp, ci = P.Microphysics1MParams(ft), P.Chen2022VelTypeIce(ft)
    st = fn(C.byref(mp.c), C.byref(ci), _abi.CMX_SNOW_SHAPE_OBLATE, 40_000, C.c_void_p(r_t.data_ptr()), C.c_void_p(q_t.data_ptr()),
            C.c_void_p(out[1:].data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == _abi.CMX_OK and torch.equal(_bits(out[1:]), _bits(full))


def test_capture_in_a_graph_and_replay(dev):
    rho, q = random_states(100_000, 13)
    r_t, q_t = torch.tensor(rho, dtype=torch.float32, device=dev), torch.tensor(q, dtype=torch.float32, device=dev)
    expect = _w("f32", r_t, q_t, "prolate")
    mp, ci = P.Microphysics1MParams("f32"), P.Chen2022VelTypeIce("f32")
    import cmx
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cmx.snow_terminal_velocity(mp, ci, r_t, q_t, cmx.Prolate(), stream=s)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        w = cmx.snow_terminal_velocity(mp, ci, r_t, q_t, cmx.Prolate(), stream=s)
    w.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(w), _bits(expect))


# ---- the column step with a shape bit -----------------------------------------------------------------------------------------------------

def _state(n_col, n_lev, ft, seed):
    from cmx import synthetic
    return [c.reshape(n_col, n_lev) for c in synthetic.mp1m_state(n_col * n_lev, dtype=DT[ft], seed=seed)]


def _inv_dz(n_lev, ft):
    g = torch.Generator().manual_seed(4)
    return (1.0 / (30.0 + 470.0 * torch.rand(n_lev, generator=g, dtype=torch.float64))).to(DT[ft])


def _column(dev, ft, cols, inv_dz, lin, opts, shape):
    import cmx
    mp, tps = P.Microphysics1MParams(ft, **opts), P.ThermodynamicsParameters(ft)
    mode, dt, nsub = (cmx.LinearizedAverage(), 40.0, 2) if lin else (cmx.Instantaneous(), None, 1)
    return cmx.column_tendencies_sedimentation_1m(mode, cmx.Microphysics1Moment(), mp, tps, P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft),
                                                  P.Chen2022VelTypeIce(ft), inv_dz, *cols, dt, nsub, snow_shape=shape)


def _check_vs_oracle(ft, got, ref, cols, lin, what):
    """dq_lcl_dt, dq_icl_dt, dq_rai_dt against the column oracle: the parity metric with the "column steps (f4)" knobs (Instantaneous) or, for
    LinearizedAverage, the same bound plus the rounding floor of the difference quotient (tests/test_mp1m_column.py _check)"""
    names = COL_NAMES[:3]
    if not lin:
        return parity.assert_parity(got, ref, parity.RTOL[ft], names=names, what=what, family="column steps (f4)")
    dt, eps = 40.0, {"f64": 2.2e-16, "f32": 1.2e-7}[ft]
    scale = sum(ref["scale"][k] for k in COL_NAMES)
    for k, q0 in zip(names, cols[3:]):
        q0 = q0.cpu().numpy().astype(np.float64).reshape(-1)
        x, r = np.asarray(got[k], dtype=np.float64), ref[k]
        tol = parity.RTOL[ft] * np.abs(r) + parity.CTOL[ft] * scale + 8 * eps * (np.abs(q0) + np.abs(r) * dt) / dt
        e = (np.abs(x - r) / np.maximum(tol, 1e-300))[~ref["near_branch"]]
        assert np.all(np.isfinite(x)) and e.max() <= 1.0, (what, k, float(e.max()))


ALT = dict(cloud_ice_formation=P.TemperatureDependent(), rain_autoconversion=P.PrescribedNd())


@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("lin", [False, True])
@pytest.mark.parametrize("shape", ["oblate", "prolate"])
@pytest.mark.parametrize("dims", [(1500, 37), (7, 300)])     # 300 levels: columns that cross the 255-point tiles of the column kernel
def test_column_step_with_a_snow_shape(dev, oracle, ft, lin, shape, dims):
    import cmx
    n_col, n_lev = dims
    cols = [c.to(dev) for c in _state(n_col, n_lev, ft, seed=17)]
    inv_dz = _inv_dz(n_lev, ft).to(dev)
    sh = _shape(shape)
    # (1) a non-default option set: shaped and unshaped run the same run-time-options kernel → the three other species bit-identical
    alt_s, alt_u = _column(dev, ft, cols, inv_dz, lin, ALT, sh), _column(dev, ft, cols, inv_dz, lin, ALT, None)
    # (2) the default options: the unshaped step runs the default-options kernel (integer exponents), the shaped one the run-time-options one
    def_s, def_u = _column(dev, ft, cols, inv_dz, lin, {}, sh), _column(dev, ft, cols, inv_dz, lin, {}, None)
    torch.cuda.synchronize()
    for k in ("dq_lcl_dt", "dq_icl_dt", "dq_rai_dt", "precip_rai"):
        assert torch.equal(getattr(alt_s, k), getattr(alt_u, k)), k
    assert not torch.equal(alt_s.dq_sno_dt, alt_u.dq_sno_dt)           # the shape does change the snow flux
    # The two instantiations differ by more than rounding: with LinearizedAverage in Float32 one well-conditioned dq_icl_dt point was 2.2e-4
    # apart, above the 2e-4 knob of "column steps (f4)".  So both are held to the column oracle (which does not depend on the snow fall speed
    # for these outputs) at those knobs, as tests/test_mp1m_column.py holds the unshaped step.
    ref = _oracle(oracle, ft, inv_dz.cpu(), [c.cpu() for c in cols], 40.0 if lin else 0.0, 2 if lin else 0)
    for what, res in (("shaped", def_s), ("unshaped", def_u)):
        got = {k: getattr(res, k).reshape(-1).cpu().numpy() for k in COL_NAMES[:3]}
        _check_vs_oracle(ft, got, ref, cols, lin, f"{what} column step, default options {ft} lin={lin}")
        np.testing.assert_allclose(res.precip_rai.cpu().numpy().astype(np.float64), ref["precip_rai"], rtol=10 * parity.RTOL[ft], atol=parity.FLOOR[ft])
    # (3) dq_sno_dt and precip_sno against the unfused composition: pointwise tendencies + the shaped w_sno + the upwind divergence in float64
    mp = P.Microphysics1MParams(ft)
    mode, dt, nsub = (cmx.LinearizedAverage(), 40.0, 2) if lin else (cmx.Instantaneous(), None, 1)
    for opts, fused in ((ALT, alt_s), ({}, def_s)):
        mpo = P.Microphysics1MParams(ft, **opts)
        pt = cmx.bulk_microphysics_tendencies_1m(mode, cmx.Microphysics1Moment(), mpo, P.ThermodynamicsParameters(ft), *[c.reshape(-1) for c in cols], dt, nsub)
        rho_p = torch.clamp(cols[0], min=0)
        q_p = torch.clamp(cols[6], min=0)
        w = cmx.snow_terminal_velocity(mp, P.Chen2022VelTypeIce(ft), rho_p.reshape(-1), q_p.reshape(-1), sh)
        torch.cuda.synchronize()
        r64, q64 = rho_p.cpu().numpy().astype(np.float64), q_p.cpu().numpy().astype(np.float64)
        F = r64 * q64 * w.reshape(n_col, n_lev).cpu().numpy().astype(np.float64)
        up = np.concatenate([F[:, 1:], np.zeros_like(F[:, :1])], axis=1)
        g = inv_dz.cpu().numpy().astype(np.float64)[None, :] / r64
        base = pt.dq_sno_dt.reshape(n_col, n_lev).cpu().numpy().astype(np.float64)
        # conditioning scale: the magnitudes summed; LinearizedAverage forms its tendency as a difference quotient (q_new − q₀)/Δt, whose terms
        # are of size |q₀|/Δt (with the default options the fused step runs the run-time-options kernel, the pointwise entry the default one)
        sc = np.abs(base) + (up + F) * g + (np.abs(cols[6].cpu().numpy().astype(np.float64)) / dt if lin else 0.0)
        ref = {"dq_sno_dt": (base + (up - F) * g).reshape(-1), "precip_sno": F[:, 0], "scale": {"dq_sno_dt": sc.reshape(-1), "precip_sno": np.abs(F[:, 0])}}
        got = {"dq_sno_dt": fused.dq_sno_dt.reshape(-1).cpu().numpy(), "precip_sno": fused.precip_sno.cpu().numpy()}
        parity.assert_parity(got, ref, parity.RTOL[ft], names=("dq_sno_dt", "precip_sno"), what=f"shaped column step vs unfused {shape} {ft} lin={lin}",
                             family="column steps (f4)", pinned_by="the unfused composition of the pointwise entries")
