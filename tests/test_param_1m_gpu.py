"""The derivatives of the 1-moment tendencies with respect to the PARAMETERS on the device (cmx_mp1m_param_jvp_* / _param_vjp_*; cmx.param_jvp_1m,
cmx.param_vjp_1m; cmx.autograd.tendencies_1m(…, theta=, names=); include/cmx.h §23): the 1-moment twin of tests/test_param_derivatives_gpu.py and
tests/test_param_autograd_gpu.py, with the reference, measure and sets of tests/param_1m_cases.py (Float64 1e-5, Float32 1e-3; the host build of the same code:
tests/test_param_1m_host.py).  param_jvp: every case on the cold, warm and limiter sets with three single states appended (whole workgroups plus a 3-point
tail); tendencies against the tendencies entry bit for bit when no size-relation exponent is moved; a column's bits against the other directions and the split;
the NaN rule.  param_vjp: the bound 2n·2⁻⁵³·Σ|t_i| that holds for any order of summation, with the terms formed exactly as in
tests/test_param_derivatives_gpu.py (one cotangent: one rounding; four: the chain in rational arithmetic up to 1025 points, the documented extra term at
262 147 on that call alone); the same bits twice; n = 0.  Graph capture; autograd."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import jacobian_1m_cases as j1
import param_1m_cases as p1
import parity
import cmx
from cmx import parameters as P
from test_param_derivatives_gpu import _eq, _fma_chain

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
NPT = {"f32": np.float32, "f64": np.float64}
FTS = ["f64", "f32"]
CASE_SETS = [(case, which) for case in p1.CASES for which in p1.SETS]
PLAIN = ("rain_autoconversion_timescale", "cloud_liquid_rain_collision_efficiency", "snow_ventilation_coefficient_b", "rain_drop_size_distribution_coefficient_n0",
         "thermal_conductivity_of_air", "latent_heat_vaporization_at_reference")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _dev_cols(cols, ft, dev):
    return [torch.from_numpy(np.array(c, dtype=np.float64)).to(DT[ft]).to(dev) for c in cols]


def _tendencies(mp, tps, x):
    return torch.stack(list(cmx.bulk_microphysics_tendencies_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), mp, tps, *x)))


def _states(n, ft, dev, which="cold", seed=0):
    rng = np.random.default_rng(seed)
    return _dev_cols([np.resize(c, n) * rng.uniform(0.9999, 1.0001, n) for c in p1.states(which)], ft, dev)


def _no_exponents(nm):
    return tuple(k for k in nm if k not in p1.EXPONENT_NAMES and k != "snow_flake_length_scale")


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case,which", CASE_SETS)
def test_param_jvp_matches_central_differences_of_the_oracle(dev, oracle, ft, case, which):
    cols = p1.reference(case, which)[0]
    n = cols[0].size
    x = _dev_cols([np.concatenate([c, e]) for c, e in zip(cols, j1.points(j1.CALLER, j1.SUITE_WARM, j1.CALLER))], ft, dev)
    mp, tps = p1.params(ft, case)
    nm = p1.names(case)
    r = cmx.param_jvp_1m(mp, tps, *x, p1.pairs(mp, case, nm), with_tendencies=True)
    S = r.jvp.cpu().numpy().transpose(1, 0, 2)
    assert np.isfinite(S).all()
    p1.assert_parity(ft, S[:, :, :n], case, which, "device param_jvp 1m")
    rest = _no_exponents(nm)
    r2 = cmx.param_jvp_1m(mp, tps, *x, p1.pairs(mp, case, rest), with_tendencies=True)
    tend = _tendencies(mp, tps, x)
    assert _eq(r2.tendencies, tend)                                              # no exponent moved: the tendencies entry's instantiation
    scale = tend.abs().amax(dim=1, keepdim=True)
    assert bool(((r.tendencies - tend).abs() <= parity.RTOL[ft] * scale).all())   # run-time flags against the default instantiation: the parity bound
    if case != "default":
        assert _eq(r.jvp[[nm.index(k) for k in rest]], r2.jvp) and _eq(r.tendencies, r2.tendencies)


@pytest.mark.parametrize("ft", FTS)
def test_a_column_does_not_depend_on_the_other_directions_or_the_split(dev, ft):
    mp, tps = p1.params(ft, "alt")
    x = _states(1025, ft, dev)
    nm = _no_exponents(p1.names("alt"))[:20]
    prs = p1.pairs(mp, "alt", nm)
    full = cmx.param_jvp_1m(mp, tps, *x, prs).jvp
    for d in (0, 7, 15, 16, 19):
        assert _eq(cmx.param_jvp_1m(mp, tps, *x, [prs[d]]).jvp[0], full[d]), nm[d]
    assert _eq(cmx.param_jvp_1m(mp, tps, *x, prs[4:20]).jvp, full[4:20])
    assert _eq(cmx.param_jvp_1m(mp, tps, *x, prs[::-1]).jvp, full.flip(0))
    zero = (mp.fam.microphysics_1m(), mp.fam.thermo())
    assert not bool(cmx.param_jvp_1m(mp, tps, *x, [zero]).jvp.any())


@pytest.mark.parametrize("ft", FTS)
def test_nan_rule(dev, ft):
    mp, tps = p1.params(ft, "default")
    x = _states(300, ft, dev, "warm")
    prs = [{k: 1.0} for k in PLAIN[:2]]
    clean = cmx.param_jvp_1m(mp, tps, *x, prs, with_tendencies=True)
    others = lambda i: torch.arange(300, device=dev) != i      # noqa: E731
    for col, i in ((0, 5), (1, 64), (6, 299)):
        y = [t.clone() for t in x]
        y[col][i] = float("nan")
        r = cmx.param_jvp_1m(mp, tps, *y, prs, with_tendencies=True)
        assert bool(torch.isnan(r.jvp[:, :, i]).all() and torch.isnan(r.tendencies[:, i]).all())
        assert _eq(r.jvp[:, :, others(i)], clean.jvp[:, :, others(i)]) and _eq(r.tendencies[:, others(i)], clean.tendencies[:, others(i)])
        v = cmx.param_vjp_1m(mp, tps, *y, [torch.ones_like(x[0])] * 4, PLAIN[:2], with_tendencies=True)
        assert bool(torch.isnan(v.grad).all() and torch.isnan(v.tendencies[:, i]).all())
    g = [torch.ones_like(x[0]) for _ in range(4)]
    g[1][17] = float("nan")
    v = cmx.param_vjp_1m(mp, tps, *x, g, PLAIN[:2], with_tendencies=True)
    assert bool(torch.isnan(v.grad).all() and torch.isnan(v.tendencies[:, 17]).all()) and _eq(v.tendencies[:, others(17)], clean.tendencies[:, others(17)])


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 262147])
def test_param_vjp_is_the_sum_of_the_jvp_columns(dev, ft, n):
    mp, tps = p1.params(ft, "default")
    x = _states(n, ft, dev, "warm", seed=n)
    prs = [{k: float(P.DEFAULT_PARAMETERS[k])} for k in PLAIN[:3]]
    S = cmx.param_jvp_1m(mp, tps, *x, prs).jvp
    gen = torch.Generator(device="cpu").manual_seed(n)
    g = [torch.randn(n, generator=gen, dtype=torch.float64).to(DT[ft]).to(dev) for _ in range(4)]
    S64, g64 = S.double().cpu().numpy(), [c.double().cpu().numpy() for c in g]
    u = 2.0 ** -53
    for o in range(4):
        cot = [g[q] if q == o else None for q in range(4)]
        v = cmx.param_vjp_1m(mp, tps, *x, cot, prs)
        terms = (g[o][None] * S[:, o]).double().cpu().numpy()
        grad = v.grad.cpu().numpy()
        assert (np.abs(grad - terms.sum(axis=1)) <= 2 * n * u * np.abs(terms).sum(axis=1)).all(), (ft, n, o, grad, terms.sum(axis=1))
        assert _eq(cmx.param_vjp_1m(mp, tps, *x, cot, prs).grad, v.grad) and _eq(cmx.param_vjp_1m(mp, tps, *x, cot, prs[1:2]).grad, v.grad[1:2])
    v = cmx.param_vjp_1m(mp, tps, *x, g, prs, with_tendencies=True)
    if n <= 1025:
        terms = np.array([[_fma_chain(ft, [g64[o][i] for o in range(4)], [S64[d, o, i] for o in range(4)]) for i in range(n)] for d in range(3)])
        bound = 2 * n * u * np.abs(terms).sum(axis=1)
    else:
        terms = sum(g64[o][None] * S64[:, o] for o in range(4))
        bound = 2 * n * u * np.abs(terms).sum(axis=1) + 3 * float(np.finfo(NPT[ft]).eps) * sum(np.abs(g64[o][None] * S64[:, o]) for o in range(4)).sum(axis=1)
    assert (np.abs(v.grad.cpu().numpy() - terms.sum(axis=1)) <= bound).all(), (ft, n, v.grad, terms.sum(axis=1), bound)
    assert _eq(v.tendencies, _tendencies(mp, tps, x))
    assert not bool(cmx.param_vjp_1m(mp, tps, *x, [None] * 4, prs).grad.any())


@pytest.mark.parametrize("ft", FTS)
def test_no_points_and_graph_capture(dev, ft):
    mp, tps = p1.params(ft, "default")
    e = [torch.empty(0, dtype=DT[ft], device=dev) for _ in range(7)]
    v = cmx.param_vjp_1m(mp, tps, *e, e[:4], PLAIN[:3])
    assert v.grad.shape == (3,) and not bool(v.grad.any())
    x = _states(4099, ft, dev, "warm")
    g = [torch.ones_like(x[0]), None, torch.full_like(x[0], -2.0), None]
    jvp, tend = torch.empty((3, 4, 4099), dtype=DT[ft], device=dev), torch.empty((4, 4099), dtype=DT[ft], device=dev)
    prs = [{k: 1.0} for k in PLAIN[:3]]
    eager_j, eager_v = cmx.param_jvp_1m(mp, tps, *x, prs, with_tendencies=True), cmx.param_vjp_1m(mp, tps, *x, g, PLAIN[:3])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cmx.param_jvp_1m(mp, tps, *x, prs, with_tendencies=True, out=(jvp, tend))
        cap_v = cmx.param_vjp_1m(mp, tps, *x, g, PLAIN[:3])
    graph.replay()
    torch.cuda.synchronize()
    assert _eq(jvp, eager_j.jvp) and _eq(tend, eager_j.tendencies) and _eq(cap_v.grad, eager_v.grad)
    x[5].mul_(1.5)
    graph.replay()
    torch.cuda.synchronize()
    assert _eq(jvp, cmx.param_jvp_1m(mp, tps, *x, prs).jvp) and _eq(cap_v.grad, cmx.param_vjp_1m(mp, tps, *x, g, PLAIN[:3]).grad) and not _eq(cap_v.grad, eager_v.grad)


@pytest.mark.parametrize("ft", FTS)
def test_autograd_theta(dev, oracle, ft):
    """loss.backward() fills theta.grad: Σ ḡ·S^ref/θ within BOUND·Σ_i Σ_o |ḡ_o,i|·s_o,i/|θ_p| over the kept states; the forward pass and the state gradients
    are those of the function without theta, bit for bit; forward mode with a tangent on theta is the param_jvp entry; TypeError / ValueError."""
    cols, S_ref, kept, dead, _, _ = p1.reference("default", "warm")
    nm = p1.names("default")
    mp, tps = p1.params(ft, "default")
    th = np.array([P.DEFAULT_PARAMETERS[k] for k in PLAIN], dtype=np.float64)
    theta = torch.tensor(th, requires_grad=True)
    x = _dev_cols(cols, ft, dev)
    for t in x[1:]:
        t.requires_grad_(True)
    g = np.random.default_rng(4).standard_normal((4, cols[0].size))
    g[:, ~kept] = 0
    w = torch.from_numpy(g).to(DT[ft]).to(dev)
    out = cmx.autograd.tendencies_1m(mp, tps, *x, theta=theta, names=PLAIN)
    sum((w[o] * out[o]).sum() for o in range(4)).backward()
    y = [t.detach().clone().requires_grad_(i > 0) for i, t in enumerate(x)]
    plain = cmx.autograd.tendencies_1m(mp, tps, *y)
    sum((w[o] * plain[o]).sum() for o in range(4)).backward()
    assert all(torch.equal(a, b) for a, b in zip(out, plain)) and all(torch.equal(a.grad, b.grad) for a, b in zip(x[1:], y[1:]))
    gq = w.double().cpu().numpy()
    ref = np.einsum("oi,opi->p", gq, S_ref[:, [nm.index(k) for k in PLAIN]]) / th
    bound = p1.BOUND[ft] * (np.abs(gq) * np.abs(S_ref).max(axis=1)).sum() / np.abs(th)
    got = theta.grad.numpy()
    print(f"theta.grad 1m {ft}: worst fraction of the bound {np.max(np.abs(got - ref) / bound):.3g}")
    assert theta.grad.dtype == torch.float64 and (np.abs(got - ref) <= bound).all(), (got, ref, bound)
    xs = [t.detach()[:300].contiguous() for t in x]
    tt = torch.linspace(-1.0, 1.0, len(PLAIN), dtype=torch.float64) * torch.tensor(th)
    with fwAD.dual_level():
        tangents = [fwAD.unpack_dual(o).tangent for o in cmx.autograd.tendencies_1m(mp, tps, *xs, theta=fwAD.make_dual(torch.tensor(th), tt), names=PLAIN)]
    fref = cmx.param_jvp_1m(mp, tps, *xs, [dict(zip(PLAIN, tt.tolist()))]).jvp[0]
    assert all(torch.equal(a, fref[o]) for o, a in enumerate(tangents))
    for bad in (torch.tensor(th).float(), torch.tensor(th).to(dev), th.tolist()):
        with pytest.raises(TypeError):
            cmx.autograd.tendencies_1m(mp, tps, *xs, theta=bad, names=PLAIN)
    edited, _ = p1.params(ft, "default")
    edited.c.rain.n0 *= 2
    with pytest.raises(ValueError):
        cmx.autograd.tendencies_1m(edited, tps, *xs, theta=torch.tensor(th), names=PLAIN)
    alt, _ = p1.params(ft, "alt")                                                # the options survive the rebuild
    assert torch.equal(cmx.autograd.tendencies_1m(alt, tps, *xs, theta=torch.tensor(th), names=PLAIN)[1], cmx.autograd.tendencies_1m(alt, tps, *xs)[1])
