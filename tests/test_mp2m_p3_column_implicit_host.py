"""The 2M + P3 column step with implicit sedimentation (include/cmx.h §24) without a GPU: every status of the new entry in the order of (9b), then `dt` — each
returned before any HIP runtime call, the column addresses below are never dereferenced —, the wrapper's refusals and public name, the code-object metadata
of the new kernel, and a self-check of the Float64 yardstick the device tests measure against (tests/p3_column_implicit_cases.py) on synthetic (a, F, w) of
eight species with an unlimited a."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

import p3_column_implicit_cases as PC
from cmx import _abi, _lib
from cmx import parameters as P

REPO = Path(__file__).resolve().parent.parent
LIB = REPO / "cloudmicrophysics.jl_amd" / "csrc" / "libcmx.so"
_OK, _BAD, _UNS = _abi.CMX_OK, _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED
SB, CHEN = _abi.CMX_P3COL_VEL_SB2006, _abi.CMX_P3COL_VEL_CHEN2022
FAKE = 4096          # a non-NULL "device address"


class _Call:
    """Default-valid arguments of cmx_mp2m_p3_column_implicit_sedimentation_<ft>; `run(**changes)` calls the entry with some replaced."""

    def __init__(self, ft, limited=True):
        self.fn = getattr(_lib.lib(), f"cmx_mp2m_p3_column_implicit_sedimentation_{ft}")
        self.mp = P.Microphysics2MParams(ft, with_ice=True, is_limited=limited)
        self.tps = P.ThermodynamicsParameters(ft)
        self.vel = P.rain_vel_params(ft)
        self.stokes = P.StokesRegimeVelType(ft)
        self.ins = (C.c_void_p * 13)(*[FAKE] * 13)
        self.outs = (C.c_void_p * 8)(*[FAKE] * 8)
        self.base = dict(wr=C.pointer(self.mp.warm_rain.c), ice=C.pointer(self.mp.ice.c), tps=C.pointer(self.tps), vel=C.pointer(self.vel), cloud=None,
                         flags=self.mp.ice.flags | SB, brent=0, p=1e-6, dt=30.0, n_col=3, n_lev=5, inv_dz=FAKE, ins=self.ins, outs=self.outs, ll=FAKE,
                         v_n=FAKE, v_m=FAKE, pr=None, pi=None)

    def run(self, **kw):
        a = dict(self.base, **kw)
        return self.fn(a["wr"], a["ice"], a["tps"], a["vel"], a["cloud"], a["flags"], a["brent"], a["p"], a["dt"], a["n_col"], a["n_lev"], a["inv_dz"],
                       a["ins"], a["outs"], a["ll"], a["v_n"], a["v_m"], a["pr"], a["pi"], None)


BAD_DTS = (-1.0, -1e-300, float("nan"), float("inf"), float("-inf"))


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_every_status_in_check_order(ft):
    """The list of tests/test_mp2m_p3_column_host.py for (9b), each with a bad dt as well: dt is looked at last."""
    c = _Call(ft)
    lim = c.mp.ice.flags
    for dt in (30.0, -1.0):
        # parameter structs, the two host arrays, the counts
        for k in ("wr", "ice", "tps", "vel", "ins", "outs"):
            assert c.run(dt=dt, **{k: None}) == _BAD, k
        assert c.run(dt=dt, n_col=-1) == _BAD
        assert c.run(dt=dt, n_lev=0) == _BAD and c.run(dt=dt, n_lev=-3) == _BAD
        # flags: an unknown bit, both or neither velocity scheme
        assert c.run(dt=dt, flags=lim | SB | _abi.CMX_P3_INPUT_IS_STATE) == _BAD
        assert c.run(dt=dt, flags=lim | SB | (1 << 10)) == _BAD
        assert c.run(dt=dt, flags=lim) == _BAD
        assert c.run(dt=dt, flags=lim | SB | CHEN) == _BAD
        # … each of these before the size rule
        huge = 16 * 0x7fffffff // 5 + 1
        assert c.run(dt=dt, flags=lim, n_col=huge) == _BAD
        # n_col · n_lev above one launch: before dt
        assert c.run(dt=dt, n_col=huge) == _UNS
        assert c.run(dt=dt, n_col=16 * 0x7fffffff + 1, n_lev=1) == _UNS
        assert c.run(dt=dt, n_col=4 * (0x7fffffff - 7) + 1, n_lev=1) == _UNS          # the collision kernel's smallest tile (4 states)
        # no columns: OK whatever the column pointers — and dt — are (the checks above still apply)
        assert c.run(dt=dt, n_col=0) == _OK
        assert c.run(dt=dt, n_col=0, inv_dz=None, ins=(C.c_void_p * 13)(), outs=(C.c_void_p * 8)(), ll=None, v_n=None, v_m=None) == _OK
        assert c.run(dt=dt, n_col=0, flags=lim) == _BAD
        # a NULL required column
        for k in ("inv_dz", "ll", "v_n", "v_m"):
            assert c.run(dt=dt, **{k: None}) == _BAD, k
        for j in range(11):
            ins = (C.c_void_p * 13)(*[FAKE] * 13)
            ins[j] = None
            assert c.run(dt=dt, ins=ins) == _BAD, j
        for j in range(8):
            outs = (C.c_void_p * 8)(*[FAKE] * 8)
            outs[j] = None
            assert c.run(dt=dt, outs=outs) == _BAD, j
        # the quantile level and the quadrature order of steps 1 and 2
        for p in (0.0, 0.5, -1e-6, float("nan")):
            assert c.run(dt=dt, p=p) == _BAD, p
        n_quad = c.mp.ice.c.quad.n
        for n in (0, _abi.CMX_QUAD_MAX + 1):
            c.mp.ice.c.quad.n = n
            assert c.run(dt=dt) == _BAD, n
        c.mp.ice.c.quad.n = n_quad
    # dt itself, on an otherwise valid call: the only refusal left, after every column check.  (A valid call is not made: it would launch.)
    for dt in BAD_DTS + ((1e39, 3.5e38) if ft == "f32" else ()):      # finite, but not as Float32
        assert c.run(dt=dt) == _BAD, dt
        assert c.run(dt=dt, n_col=0) == _OK, dt
        assert c.run(dt=dt, n_col=16 * 0x7fffffff // 5 + 1) == _UNS, dt


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_parameter_domain_checks_come_before_dt(ft):
    """The limited rain PSD needs ordered limiter pairs, the not-limited SB2006 fall speed aR < bR — as for (9b), with a good and with a bad dt."""
    c = _Call(ft, limited=False)
    for dt in (30.0, float("nan")):
        assert c.run(dt=dt, flags=c.mp.ice.flags | SB | _abi.CMX_P3_RAIN_PDF_LIMITED) == _BAD
        aR = c.vel.sb2006.aR
        c.vel.sb2006.aR = c.vel.sb2006.bR
        assert c.run(dt=dt) == _BAD
        c.vel.sb2006.aR = aR


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: the wrapper's checks run, the library is never reached."""
    @property
    def is_cuda(self):
        return True


def _cols(ft, n_col=4, n_lev=6):
    dt = torch.float32 if ft == "f32" else torch.float64
    return [torch.ones(n_col, n_lev, dtype=dt).as_subclass(_FakeCuda) for _ in range(11)], torch.ones(n_lev, dtype=dt).as_subclass(_FakeCuda)


def test_wrapper_type_and_value_errors():
    import cmx
    ft = "f32"
    cols, inv_dz = _cols(ft)
    mp, tps = P.Microphysics2MParams(ft, with_ice=True), P.ThermodynamicsParameters(ft)
    f = cmx.column_implicit_sedimentation_2m_p3
    for dt in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dt must be"):
            f(mp, tps, inv_dz, *cols, dt)
    with pytest.raises(TypeError):
        f(mp, tps, inv_dz, *cols)                                                           # no dt
    # dt is judged last, as the C entry does: with a bad dt the refusals below are what they are with a good one
    with pytest.raises(TypeError):
        f(P.Microphysics2MParams(ft), tps, inv_dz, *cols, float("nan"))
    with pytest.raises(ValueError, match="inv_dz"):
        f(mp, tps, inv_dz[:5], *cols, -1.0)
    with pytest.raises(TypeError):
        f(P.Microphysics2MParams(ft), tps, inv_dz, *cols, 30.0)                             # no ice parameters
    with pytest.raises(TypeError):
        f(P.WarmRainParams2M(ft), tps, inv_dz, *cols, 30.0)
    with pytest.raises(TypeError):
        f(P.Microphysics2MParams("f64", with_ice=True), tps, inv_dz, *cols, 30.0)           # float type of the parameters
    with pytest.raises(TypeError):
        f(mp, P.ThermodynamicsParameters("f64"), inv_dz, *cols, 30.0)
    with pytest.raises(TypeError):
        f(mp, tps, inv_dz, *cols, 30.0, cloud_vel=P.StokesRegimeVelType("f64"))
    with pytest.raises(TypeError):
        f(mp, tps, inv_dz, *cols, 30.0, vel_params=P.rain_vel_params("f64"))
    with pytest.raises(TypeError):
        f(mp, tps, inv_dz, *cols, 30.0, vel=object())
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols, 30.0, vel=None)                                           # the column step needs a rain fall-speed scheme
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz[:5], *cols, 30.0)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz.double(), *cols, 30.0)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *[c.reshape(-1) for c in cols], 30.0)                            # not (n_col, n_lev)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols[:10], cols[10][:, :5], 30.0)                               # a column of another shape
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols[:10], cols[10].double(), 30.0)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols[:10], cols[10].t().contiguous().t(), 30.0)                 # not contiguous
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols, 30.0, log_lambda_guess=cols[0][:, :5])
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols, 30.0, inpc_log_shift=cols[0].double())
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *[torch.ones(4, 6) for _ in range(11)], 30.0)                    # not on the GPU
    mixed = P.Microphysics2MParams(ft, with_ice=True)
    mixed.ice = P.P3IceParams(ft, is_limited=False)
    with pytest.raises(ValueError):
        f(mixed, tps, inv_dz, *cols, 30.0)                                                  # warm_rain and ice disagree on is_limited
    bad_out = cmx.ColumnTendencies2MP3(*[torch.ones(4, 6).as_subclass(_FakeCuda) for _ in range(10)], torch.ones(4, 5).as_subclass(_FakeCuda), None, None)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols, 30.0, out=bad_out)
    bad_pf = cmx.ColumnTendencies2MP3(*[torch.ones(4, 6).as_subclass(_FakeCuda) for _ in range(11)], torch.ones(3).as_subclass(_FakeCuda), None)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols, 30.0, out=bad_pf)


def test_public_names():
    import inspect

    import cmx
    assert cmx.column_implicit_sedimentation_2m_p3 is cmx.bulk_tendencies.column_implicit_sedimentation_2m_p3
    assert "column_implicit_sedimentation_2m_p3" in getattr(cmx, "__all__", dir(cmx))
    # the keywords of the explicit step, and dt as the last positional argument
    new, old = (inspect.signature(g).parameters for g in (cmx.column_implicit_sedimentation_2m_p3, cmx.column_tendencies_sedimentation_2m_p3))
    assert [n for n in new if n != "dt"] == list(old) and list(new)[14] == "dt"
    assert all(new[n].kind == old[n].kind and new[n].default == old[n].default for n in old)
    assert inspect.signature(cmx.column_implicit_sedimentation_2m_p3).return_annotation == inspect.signature(cmx.column_tendencies_sedimentation_2m_p3).return_annotation


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", REPO / "tools" / "kernel_resources.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_new_kernel_spills_nothing_and_touches_no_scratch():
    """Every mp2m_p3_implicit_sedimentation_kernel instantiation of the cross-compiled library — {limited} × {SB2006, Chen, Chen general Γ} × {cloud} × {f32, f64}:
    no spilled vector register and no scratch instruction anywhere (tests/test_kernel_resources.py asserts the absence of scratch for the library as a whole; here
    it is shown that the new kernels were found and their loops parsed), and what that test does not look at: G is written over B, so that the Float64
    instantiations — A and B/G of 256 points × 8 species, the carry, the exp2 / log2 tables — stay inside 40 KiB and four workgroups share a CU's 160 KiB."""
    assert LIB.exists(), "libcmx.so is not built"
    tool = _tool()
    ks = tool.kernels(str(LIB))
    new = [k for k in ks if "mp2m_p3_implicit_sedimentation_kernel" in k["name"]]
    assert len(new) == 24, len(new)
    scr = tool.scratch_in_loops(str(LIB), "mp2m_p3_implicit_sedimentation_kernel")
    assert len(scr) == len(new)
    for k in new:
        print(f"vgpr {k['vgpr']:3d} sgpr spill {k['sgpr_spill']:3d} private {k['private']:3d} B lds {k['lds']:5d} B  {tool.demangle([k['name']])[0][:120]}")
        assert k["vgpr_spill"] == 0, k
        f64 = "IdLb" in k["name"]
        assert k["lds"] <= (40 if f64 else 20) * 1024, k
        n, inside, innermost, n_loops = scr[k["name"]]
        assert n_loops >= 2, (k["name"], n_loops)      # the disassembly was parsed: the chunk loop and the chain are there
        assert n == 0, (k["name"], n)


@pytest.mark.parametrize("dt", PC.DTS)
def test_the_yardstick_on_eight_species_with_an_unlimited_tendency(dt):
    """The NumPy recipe on synthetic (a, F, w) — Δz ∈ [30, 500] m, w up to 12 m/s, a between −3 χ/Δt and +χ/Δt in half the cells — satisfies the identity, the
    surface relation, the budget and the lower bound within the multiples the device tests use, at eps(Float64); the recipe stays within 2.3 eps·scale of the
    lower bound on (37, 20); the explicit combination on the same input falls below it in a good share of the falling cells at Δt = 300."""
    eps = PC.EPS["f64"]
    for seed, (n_col, n_lev) in enumerate([(37, 20), (5, 64), (3, 85), (2, 600), (7, 1)]):
        s = PC.synthetic(seed, n_col, n_lev, dt)
        assert s["a"].shape[0] == 8 and (s["chi"] + dt * s["a"] < 0).mean() > 0.2      # unlimited: what SC.synthetic never produces
        out, G, c, beta, g = PC.recipe(s["a"], s["F"], s["w"], s["rho"], s["inv_dz"], dt)
        assert np.isfinite(out).all()
        if dt == 300.0 and n_lev > 1:
            assert c.max() > 20.0
        expl = PC.explicit(s["a"], s["F"], s["rho"], s["inv_dz"])
        res, S = PC.identity(out, expl, s["a"], s["F"], c, beta, g)
        assert (res <= PC.M_IDENTITY * eps * S).all(), float((res / S.clip(1e-300)).max() / eps)
        res, sc = PC.surface(G[..., 0], s["F"][..., 0], beta[..., 0], out[..., 0], c[..., 0], s["a"][..., 0])
        assert (res <= PC.M_IDENTITY * eps * sc).all()
        res, sc = PC.budget(out, G[..., 0], s["a"], s["rho"], s["inv_dz"])
        assert (res <= PC.M_BUDGET * eps * sc).all(), float((res / sc.clip(1e-300)).max() / eps)
        margin, sc, m = PC.lower_bound_margin(s["chi"], out, s["a"], s["F"], s["w"], s["rho"], s["inv_dz"], dt)
        worst = float((-margin / sc.clip(1e-300)).max() / eps)
        assert (margin >= -m * eps * sc).all(), worst
        if (n_col, n_lev) == (37, 20):
            print(f"dt={dt:g}: the recipe's worst shortfall against the lower bound on (37, 20): {worst:.3g} eps·scale")
            assert worst <= 2.3, worst
        # the bound is not empty: it is attained (p < 0 at a column top gives equality to rounding) …
        top_neg = (s["chi"] + dt * s["a"])[..., -1] < 0
        assert top_neg.any() and (np.abs(margin[..., -1][top_neg]) <= m[..., -1][top_neg] * eps * sc[..., -1][top_neg]).all()
        # … and the explicit combination falls below it where c > 1
        if dt == 300.0 and n_lev > 1:
            falling = s["w"] > 0
            em = PC.lower_bound_margin(s["chi"], expl, s["a"], s["F"], s["w"], s["rho"], s["inv_dz"], dt)[0]
            assert ((em < -m * eps * sc) & falling).sum() >= 0.1 * falling.sum()


def test_the_lower_bound_is_zero_without_deficits_and_the_recipe_carries_nan_downward_only():
    """χ + Δt a ≥ 0 everywhere: p⁻ = 0, G⁻ = 0, L = 0 — the positivity of §21.  A NaN in a at level k reaches the levels ≤ k of its species and column only."""
    s = PC.synthetic(11, 3, 20, 30.0)
    a = np.abs(s["a"])
    assert (PC.lower_bound(s["chi"], a, s["w"], s["rho"], s["inv_dz"], 30.0) == 0).all()
    clean = PC.recipe(s["a"], s["F"], s["w"], s["rho"], s["inv_dz"], 30.0)[0]
    bad = s["a"].copy()
    bad[6, 1, 7] = np.nan
    out = PC.recipe(bad, s["F"], s["w"], s["rho"], s["inv_dz"], 30.0)[0]
    hit = np.zeros(out.shape, dtype=bool)
    hit[6, 1, :8] = True
    assert np.isnan(out[hit]).all() and (out[~hit] == clean[~hit]).all()
