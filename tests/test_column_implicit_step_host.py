"""The column steps with backward-Euler sedimentation (include/cmx.h §21) without a GPU: the statuses of the four entries and their order — those of the
§20 entries, every refused call returns before anything is launched —, the wrappers' Python-side errors, the code-object metadata of the new kernels, and a
self-check of the Float64 recipe the device tests measure against (tests/column_implicit_step_cases.py)."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

import column_implicit_step_cases as SC
import cmx
from cmx import _abi, _lib
from cmx import parameters as P

REPO = Path(__file__).resolve().parent.parent
LIB = REPO / "cloudmicrophysics.jl_amd" / "csrc" / "libcmx.so"
OK, BAD, UNSUPPORTED = _abi.CMX_OK, _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED
HUGE = 16 * 0x7fffffff      # kMaxPoints (csrc/cmx_launch.hpp)
FAKE = C.c_void_p(4096)     # a non-NULL pointer that no refused call dereferences
ENTRIES = ["implicit_step", "implicit_average_sedimentation"]      # the second: the §20 entry gives the same answer to every call below


def _sb2006(ft, entry="implicit_step", **kw):
    """The status of cmx_sb2006_column_<entry>_<ft> for a valid call with the given arguments replaced."""
    wr, tps, vel = P.WarmRainParams2M(ft), P.ThermodynamicsParameters(ft), P.rain_vel_params(ft)
    a = dict(wr=C.byref(wr.c), tps=C.byref(tps), vel=C.byref(vel), cloud=None, flags=_abi.CMX_SB2006_LIMITED | _abi.CMX_VEL_SB2006, dt=30.0, nsub=2,
             step=_abi.CMX_STEP_NONNEGATIVE, n_col=8, n_lev=64, inv_dz=FAKE, cols=[FAKE] * 7, out=[FAKE] * 4, precip=None)
    a.update(kw)
    fn = getattr(_lib.lib(), f"cmx_sb2006_column_{entry}_{ft}")
    return fn(a["wr"], a["tps"], a["vel"], a["cloud"], a["flags"], a["dt"], a["nsub"], a["step"], a["n_col"], a["n_lev"], a["inv_dz"], *a["cols"], *a["out"],
              a["precip"], None)


def _mp1m(ft, entry="implicit_step", **kw):
    """The status of cmx_mp1m_column_<entry>_<ft> for a valid call with the given arguments replaced."""
    mp, tps = P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft)
    st, cr, ci = P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft), P.Chen2022VelTypeIce(ft)
    a = dict(mp=C.byref(mp.c), tps=C.byref(tps), stokes=C.byref(st), chen_rain=C.byref(cr), chen_ice=C.byref(ci), flags=mp.flags, dt=30.0, nsub=2,
             step=_abi.CMX_STEP_NONNEGATIVE, n_col=8, n_lev=64, inv_dz=FAKE, cols=[4096] * 7, out=[4096] * 4, precip_rai=None, precip_sno=None)
    a.update(kw)
    tab = lambda ps: (C.c_void_p * len(ps))(*ps) if ps is not None else None  # noqa: E731
    fn = getattr(_lib.lib(), f"cmx_mp1m_column_{entry}_{ft}")
    return fn(a["mp"], a["tps"], a["stokes"], a["chen_rain"], a["chen_ice"], a["flags"], a["dt"], a["nsub"], a["step"], a["n_col"], a["n_lev"], a["inv_dz"],
              tab(a["cols"]), tab(a["out"]), a["precip_rai"], a["precip_sno"], None)


BAD_STEPS = [dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(nsub=0), dict(nsub=65), dict(nsub=-1), dict(step=2),
             dict(step=_abi.CMX_STEP_NONNEGATIVE | 4)]


def _sb2006_calls(ft):
    """(arguments, expected status) of the 2-moment entry: the list of tests/test_column_implicit_average_host.py."""
    bad = P.WarmRainParams2M(ft)
    bad.c.seifert_beheng.pdf_r.lambda_min, bad.c.seifert_beheng.pdf_r.lambda_max = 1e4, 1e3
    vel = P.rain_vel_params(ft)
    vel.sb2006.aR = vel.sb2006.bR
    lim, sb, chen = _abi.CMX_SB2006_LIMITED, _abi.CMX_VEL_SB2006, _abi.CMX_VEL_CHEN2022
    calls = [({k: None}, BAD) for k in ("wr", "tps", "vel")]
    calls += [(dict(n_lev=0), BAD), (dict(n_lev=-3), BAD), (dict(n_col=-1), BAD)]
    calls += [(dict(flags=lim | sb | (1 << 9)), BAD), (dict(flags=lim), BAD), (dict(flags=sb | chen), BAD)]
    calls += [(dict(inv_dz=None), BAD)]
    calls += [(dict(cols=[None if i == j else FAKE for i in range(7)]), BAD) for j in range(7)]
    calls += [(dict(out=[None if i == j else FAKE for i in range(4)]), BAD) for j in range(4)]
    calls += [(dict(wr=C.byref(bad.c)), BAD), (dict(vel=C.byref(vel), flags=sb), BAD)]
    calls += [(b, BAD) for b in BAD_STEPS + ([dict(dt=2e-38, nsub=64), dict(dt=1e39)] if ft == "f32" else [])]
    # the order: n = 0 is CMX_OK once the structs, the flags and the counts are valid — before the columns, the tables and the step are looked at …
    calls += [(dict(n_col=0, inv_dz=None, cols=[None] * 7, out=[None] * 4, wr=C.byref(bad.c), dt=-1.0, nsub=0, step=8), OK)]
    # … but after the flags and the structs; a point count no launch expresses is CMX_ERR_UNSUPPORTED before the columns and the step, after the flags
    calls += [(dict(n_col=0, flags=lim), BAD), (dict(n_col=0, tps=None), BAD)]
    calls += [(dict(n_col=HUGE // 64 + 1, cols=[None] * 7, dt=-1.0), UNSUPPORTED), (dict(n_col=HUGE // 64 + 1, flags=0), BAD)]
    calls += [(dict(n_col=HUGE // 64, cols=[None] * 7), BAD)]      # the largest count passes the limit and fails on its columns
    return calls, (bad, vel)      # (the structs stay alive with the list)


def _mp1m_calls(ft):
    flags = P.Microphysics1MParams(ft).flags
    obl, pro = _abi.CMX_1M_SED_SNOW_OBLATE, _abi.CMX_1M_SED_SNOW_PROLATE
    calls = [({k: None}, BAD) for k in ("mp", "tps", "stokes", "chen_rain", "chen_ice")]
    calls += [(dict(n_lev=0), BAD), (dict(n_col=-1), BAD)]
    # the snow shapes: both bits are a bad argument as in the existing entry, a single one is not done here
    calls += [(dict(flags=flags | obl | pro), BAD), (dict(flags=flags | obl), UNSUPPORTED), (dict(flags=flags | pro), UNSUPPORTED)]
    calls += [(dict(inv_dz=None), BAD), (dict(cols=None), BAD), (dict(out=None), BAD)]
    calls += [(dict(cols=[None if i == j else 4096 for i in range(7)]), BAD) for j in range(7)]
    calls += [(dict(out=[None if i == j else 4096 for i in range(4)]), BAD) for j in range(4)]
    calls += [(b, BAD) for b in BAD_STEPS + ([dict(dt=2e-38, nsub=64), dict(dt=1e39)] if ft == "f32" else [])]
    # the order: the shape bits before everything but the structs and the counts; n = 0 before the columns and the step; the launch limit before both
    calls += [(dict(flags=flags | obl, n_col=0, cols=None, dt=-1.0), UNSUPPORTED), (dict(flags=flags | obl, mp=None), BAD)]
    calls += [(dict(n_col=0, inv_dz=None, cols=None, out=None, dt=-1.0, nsub=0, step=8), OK), (dict(n_col=0, tps=None), BAD)]
    calls += [(dict(n_col=HUGE // 64 + 1, cols=None, dt=-1.0), UNSUPPORTED), (dict(n_col=HUGE // 64, cols=None), BAD)]
    return calls


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_sb2006_statuses_and_their_order_without_gpu(ft):
    """Every refused call, with its status — and the §20 entry answers each of them the same: the same checks in the same order."""
    calls, _keep = _sb2006_calls(ft)
    assert len(calls) > 30
    for kw, want in calls:
        assert _sb2006(ft, **kw) == want, kw
        assert _sb2006(ft, ENTRIES[1], **kw) == want, kw


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_mp1m_statuses_and_their_order_without_gpu(ft):
    calls = _mp1m_calls(ft)
    assert len(calls) > 30
    for kw, want in calls:
        assert _mp1m(ft, **kw) == want, kw
        assert _mp1m(ft, ENTRIES[1], **kw) == want, kw
    flags = P.Microphysics1MParams(ft).flags | (1 << 30)      # an unknown option bit: whatever the tendencies entry answers (check_flags_1m), not CMX_OK
    assert _mp1m(ft, flags=flags) < 0 and _mp1m(ft, flags=flags) == _mp1m(ft, ENTRIES[1], flags=flags)


def test_the_wrappers_python_side_errors_without_gpu():
    """Everything the wrappers refuse before they touch the device, on host tensors."""
    ft, shape = "f32", (4, 16)
    cols = [torch.rand(shape) for _ in range(7)]
    inv_dz = torch.rand(shape[1])
    mp2, mp1, tps = P.Microphysics2MParams(ft), P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft)
    vels = (P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft), P.Chen2022VelTypeIce(ft))
    two = lambda c=cols, dt=30.0, nsub=2, **kw: cmx.column_implicit_step_2m(mp2, tps, inv_dz, *c, dt, nsub, **kw)  # noqa: E731
    one = lambda c=cols, dt=30.0, nsub=2, **kw: cmx.column_implicit_step_1m(mp1, tps, *vels, inv_dz, *c, dt, nsub, **kw)  # noqa: E731
    for call in (two, one):
        for bad in (dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(nsub=0), dict(nsub=65), dict(nsub=1.5), dict(nsub=True)):
            with pytest.raises(ValueError, match="dt must be|nsub must be"):
                call(**bad)
    tr = [c.clone() for c in cols]
    tr[3] = cols[3].t().contiguous().t()
    with pytest.raises(ValueError, match="q_lcl must be a contiguous"):
        one(tr)
    with pytest.raises(ValueError, match="shape"):
        one([c.reshape(-1) for c in cols])
    with pytest.raises(ValueError, match="q_rai: shape"):
        one(cols[:5] + [cols[5].reshape(shape[1], shape[0])] + cols[6:])
    # … and there is no CPU path
    with pytest.raises(ValueError, match="resident on the GPU"):
        one()
    with pytest.raises(ValueError, match="resident on the GPU"):
        two()
    with pytest.raises(TypeError):
        cmx.column_implicit_step_2m(mp1, tps, inv_dz, *cols, 30.0)      # not a 2-moment parameter set
    with pytest.raises(TypeError):
        cmx.column_implicit_step_1m(mp2, tps, *vels, inv_dz, *cols, 30.0)


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", REPO / "tools" / "kernel_resources.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_new_kernels_spill_nothing_and_touch_no_scratch():
    """Every implicit_sedimentation_step_kernel instantiation of the cross-compiled library: no spilled vector register, no scratch instruction, and the LDS
    of the three [256][4] arrays and the carry (Float64: plus the exp2 / log2 tables) far inside a workgroup's 64 KiB.  The name matches none of the
    fragments by which the existing tests select kernels."""
    assert LIB.exists(), "libcmx.so is not built"
    tool = _tool()
    ks = tool.kernels(str(LIB))
    new = [k for k in ks if "implicit_sedimentation_step_kernel" in k["name"]]
    assert len(new) == 12, len(new)      # SB2006: {limited} x {integer exponents}; 1-moment: {default, run-time flags}; each x {f32, f64}
    frags = ("sb2006_column_kernel", "mp1m_column_kernel", "implicit_average_kernel", "implicit_average_column_kernel")
    for k in new:
        assert not any(frag in k["name"] for frag in frags), k["name"]
    assert len([k for k in ks if "implicit_average_column_kernel" in k["name"]]) == 12      # the §20 kernels are all still there
    scr = tool.scratch_in_loops(str(LIB), "implicit_sedimentation_step_kernel")
    assert len(scr) == len(new)
    for k in new:
        print(f"vgpr {k['vgpr']:3d} sgpr spill {k['sgpr_spill']:3d} private {k['private']:3d} B lds {k['lds']:5d} B  {tool.demangle([k['name']])[0][:150]}")
        assert k["vgpr_spill"] == 0, k
        assert 3 * 256 * 4 * 4 <= k["lds"] <= 32 * 1024, k
        n, inside, innermost, n_loops = scr[k["name"]]
        assert n_loops >= 3, (k["name"], n_loops)      # the disassembly was parsed: the chunk loop, the substep loop and the chain are there
        assert n == 0, (k["name"], n)


@pytest.mark.parametrize("dt", SC.DTS)
def test_the_float64_recipe_satisfies_what_the_device_tests_assert(dt):
    """The yardstick itself: the NumPy recipe on synthetic (a, F, w) — Δz ∈ [30, 500] m, w up to 9 m/s, so c up to 90 at Δt = 300 — satisfies the identity, the
    surface relation, the budget and positivity within the bounds the device tests use, at eps(Float64); and the explicit combination on the same input goes
    negative where c > 1."""
    eps = SC.EPS["f64"]
    for seed, (n_col, n_lev) in enumerate([(5, 64), (3, 85), (2, 600), (7, 1)]):
        s = SC.synthetic(seed, n_col, n_lev, dt)
        out, G, c, beta, g = SC.recipe(s["a"], s["F"], s["w"], s["rho"], s["inv_dz"], dt)
        assert np.isfinite(out).all() and G.min() >= -8 * eps * s["F"].max()      # (β a + F = 0 to rounding where the limiter emptied a cell)
        if dt == 300.0 and n_lev > 1:
            assert c.max() > 20.0
        expl = SC.explicit(s["a"], s["F"], s["rho"], s["inv_dz"])
        res, S = SC.identity(out, expl, s["a"], s["F"], c, beta, g)
        assert (res <= SC.M_IDENTITY * eps * S).all(), float((res / S.clip(1e-300)).max() / eps)
        res, sc = SC.surface(G[..., 0], s["F"][..., 0], beta[..., 0], out[..., 0])
        assert (res <= SC.M_IDENTITY * eps * sc).all()
        res, sc = SC.budget(out, G[..., 0], s["a"], s["rho"], s["inv_dz"])
        assert (res <= SC.M_BUDGET * eps * sc).all(), float((res / sc.clip(1e-300)).max() / eps)
        new, sc = SC.positivity(s["chi"], out, s["a"], s["F"], beta, g, dt)
        assert (new >= -SC.m_positivity(c) * eps * sc).all()
        if dt == 300.0 and n_lev > 1:
            fast = c > 1.0
            assert ((s["chi"] + dt * expl < 0) & fast).sum() > 0.25 * fast.sum()      # the prototype: about half


def test_the_recipe_is_the_explicit_step_without_levels_and_carries_nan_downward_only():
    """inv_dz = 0: out = a and G = fma(β, a, F); a NaN in a at level k reaches the levels ≤ k of its species and column, nothing else."""
    s = SC.synthetic(11, 3, 20, 30.0)
    out, G, c, beta, g = SC.recipe(s["a"], s["F"], s["w"], s["rho"], 0.0 * s["inv_dz"], 30.0)
    assert (out == s["a"]).all() and (G == beta * s["a"] + s["F"]).all()
    clean = SC.recipe(s["a"], s["F"], s["w"], s["rho"], s["inv_dz"], 30.0)[0]
    a = s["a"].copy()
    a[2, 1, 7] = np.nan
    out = SC.recipe(a, s["F"], s["w"], s["rho"], s["inv_dz"], 30.0)[0]
    hit = np.zeros(out.shape, dtype=bool)
    hit[2, 1, :8] = True
    assert np.isnan(out[hit]).all() and (out[~hit] == clean[~hit]).all()
