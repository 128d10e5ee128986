"""The derivatives of the SB2006 warm-rain tendencies with respect to the PARAMETERS on the device (cmx_sb2006_warm_rain_param_jvp_* / _param_vjp_*;
cmx.warm_rain_param_jvp_2m, cmx.warm_rain_param_vjp_2m; include/cmx.h §22).  tests/param_cases.py has the parameters, the reference (central differences of the
Float64 oracle with respect to one ClimaParams name at a time, as logarithmic sensitivities), the measure and the bounds (Float64 1e-5, Float32 1e-3); the host
build of the same code is checked in tests/test_param_derivatives_host.py.

param_jvp: the interior set and the limiter set with three single states appended (n = 4099 / 515: whole workgroups plus a 3-point tail), every case; the
tendencies against the tendencies entry bit for bit when no exponent direction is present; a column's bits against co-requested directions, ndir = 1 against 16
and the split into calls; the NaN rule.
param_vjp: against a float64 numpy sum of ḡ·(the device's own param_jvp columns) with the bound that holds for ANY order of summation of n terms in double,
|grad − ref| ≤ 2n·2⁻⁵³·Σ_i|t_i| (Higham, Accuracy and Stability, §4.2: γ_{n−1} ≤ 2n·u for n·u < 1/2).  The terms t_i are what the device adds: with ONE
cotangent column t_i = ḡ_i·S_i rounded once to the float type, which numpy forms exactly; with several cotangents t_i is a chain of fused multiply-adds in the
float type, which the test forms exactly in rational arithmetic up to 1025 points.  In both the bound is asserted as it stands.  At 262 147 points the rational
chain is too slow for a test: there the four-cotangent call alone gets (NOUT − 1)·eps(FT)·Σ_o|ḡ_o S_o| added, and the single-cotangent calls hold the strict bound.
Sizes 1 … 262 147 (more points than partials × lanes: a lane adds more than one point); two calls give the same bits; NULL cotangent
members; n = 0.  Both entries inside a graph capture on one stream."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import jacobian_cases as jc
import param_cases as pc
import parity
import cmx
from cmx import _abi, _lib
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
NPT = {"f32": np.float32, "f64": np.float64}
FTS = ["f64", "f32"]
CASES = [(limited, perturbed, which) for which in ("interior", "limiters") for limited in (True, False) for perturbed in (False, True)]
NO_EXPONENTS = tuple(k for k in pc.NAMES if k not in pc.EXPONENTS)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _dev_cols(cols, ft, dev):
    return [torch.from_numpy(np.array(c, dtype=np.float64)).to(DT[ft]).to(dev) for c in cols]      # (copies: the references are read-only)


def _eq(a, b):
    """Same bits, NaN = NaN."""
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


def _pairs(wr, names, perturbed):
    return [P.parameter_direction(wr, {k: float(t)}) for k, t in zip(names, pc.theta(perturbed, names))]


def _tendencies(wr, tps, cols):
    return torch.stack(list(cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), wr, tps, *cols))[:4])


def _states(n, ft, dev, seed=0):
    """n states: the interior set repeated, every column scaled by a factor within 1 ± 1e-3 per point so that no two points are the same."""
    rng = np.random.default_rng(seed)
    return _dev_cols([np.resize(c, n) * rng.uniform(0.999, 1.001, n) for c in pc.states("interior")], ft, dev)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("limited,perturbed,which", CASES)
def test_param_jvp_matches_central_differences_of_the_oracle(dev, oracle, ft, limited, perturbed, which):
    cols = pc.reference(limited, perturbed, which)[0]
    n = cols[0].size
    cols3 = [np.concatenate([c, e]) for c, e in zip(cols, jc.points(jc.WARM_RAIN, jc.KAT, jc.BOUNDARY))]      # whole workgroups and a tail of three lanes
    wr, tps = pc.params(ft, limited, pc.overrides(perturbed))
    x = _dev_cols(cols3, ft, dev)
    r = cmx.warm_rain_param_jvp_2m(wr, tps, *x, _pairs(wr, pc.NAMES, perturbed), with_tendencies=True)
    S = r.jvp.cpu().numpy().transpose(1, 0, 2)
    assert np.isfinite(S).all()
    pc.assert_parity(ft, S[:, :, :n], limited, perturbed, which, "device param_jvp")
    # no exponent direction: the instantiation of the tendencies entry, whose tendencies these are bit for bit (the first call above held one: parity bound)
    r2 = cmx.warm_rain_param_jvp_2m(wr, tps, *x, _pairs(wr, NO_EXPONENTS, perturbed), with_tendencies=True)
    tend = _tendencies(wr, tps, x)
    assert _eq(r2.tendencies, tend)
    scale = tend.abs().amax(dim=1, keepdim=True)
    assert bool(((r.tendencies - tend).abs() <= parity.RTOL[ft] * scale).all())      # general against integer exponents: the parity bound of the float type
    if perturbed:      # both calls ran the general instantiation: the columns are the same bits whatever else was requested
        keep = [pc.NAMES.index(k) for k in NO_EXPONENTS]
        assert _eq(r.jvp[keep], r2.jvp) and _eq(r.tendencies, r2.tendencies)


@pytest.mark.parametrize("ft", FTS)
def test_a_column_does_not_depend_on_the_other_directions_or_the_split(dev, ft):
    wr, tps = pc.params(ft, True, {})
    x = _states(1025, ft, dev)
    names = NO_EXPONENTS[:20]
    pairs = _pairs(wr, names, False)
    full = cmx.warm_rain_param_jvp_2m(wr, tps, *x, pairs).jvp               # 16 + 4 directions: two calls of the entry
    for d in (0, 7, 15, 16, 19):
        assert _eq(cmx.warm_rain_param_jvp_2m(wr, tps, *x, [pairs[d]]).jvp[0], full[d]), names[d]      # ndir = 1
    assert _eq(cmx.warm_rain_param_jvp_2m(wr, tps, *x, pairs[4:20]).jvp, full[4:20])                    # ndir = 16, other neighbours
    assert _eq(cmx.warm_rain_param_jvp_2m(wr, tps, *x, pairs[::-1]).jvp, full.flip(0))
    # NULL members of the jvp table through the raw ABI: the columns that are written are the same bits, the others untouched
    out = torch.full((2, 4, 1025), 7.0, dtype=DT[ft], device=dev)
    fam = wr.fam
    d_wr, d_tps = (fam.warm_rain_2m * 2)(pairs[3][0], pairs[9][0]), (fam.thermo * 2)(pairs[3][1], pairs[9][1])
    table = (C.c_void_p * 8)(*[out[d, o].data_ptr() if (d, o) in ((0, 1), (1, 2)) else None for d in range(2) for o in range(4)])
    _lib.call("cmx_sb2006_warm_rain_param_jvp", fam, dev, C.byref(wr.c), C.byref(tps), 1, 1025, *[C.c_void_p(t.data_ptr()) for t in x], 2, d_wr, d_tps, table, None)
    torch.cuda.synchronize()
    assert _eq(out[0, 1], full[3, 1]) and _eq(out[1, 2], full[9, 2])
    assert bool((out[0, 0] == 7).all() and (out[0, 2:] == 7).all() and (out[1, :2] == 7).all() and (out[1, 3] == 7).all())
    # a zero direction: zeros
    zero = (fam.warm_rain_2m(), fam.thermo())
    assert not bool(cmx.warm_rain_param_jvp_2m(wr, tps, *x, [zero]).jvp.any())


@pytest.mark.parametrize("ft", FTS)
def test_nan_rule(dev, ft):
    wr, tps = pc.params(ft, True, {})
    x = _states(300, ft, dev)
    pairs = _pairs(wr, ("SB2006_collection_kernel_coeff_kcc", "SB2006_collection_kernel_coeff_kcr"), False)
    clean = cmx.warm_rain_param_jvp_2m(wr, tps, *x, pairs, with_tendencies=True)
    for col, i in ((0, 5), (1, 64), (4, 299)):
        y = [t.clone() for t in x]
        y[col][i] = float("nan")
        r = cmx.warm_rain_param_jvp_2m(wr, tps, *y, pairs, with_tendencies=True)
        assert bool(torch.isnan(r.jvp[:, :, i]).all() and torch.isnan(r.tendencies[:, i]).all())
        others = torch.arange(300, device=dev) != i
        assert _eq(r.jvp[:, :, others], clean.jvp[:, :, others]) and _eq(r.tendencies[:, others], clean.tendencies[:, others])
        g = [torch.ones_like(x[0])] * 4
        v = cmx.warm_rain_param_vjp_2m(wr, tps, *y, g, pairs, with_tendencies=True)
        assert bool(torch.isnan(v.grad).all() and torch.isnan(v.tendencies[:, i]).all()) and _eq(v.tendencies[:, others], clean.tendencies[:, others])
    g = [torch.ones_like(x[0]) for _ in range(4)]
    g[2][17] = float("nan")                                                      # a NaN cotangent: the sum is NaN, and that point's tendencies
    v = cmx.warm_rain_param_vjp_2m(wr, tps, *x, g, pairs, with_tendencies=True)
    assert bool(torch.isnan(v.grad).all() and torch.isnan(v.tendencies[:, 17]).all())
    assert _eq(v.tendencies[:, torch.arange(300, device=dev) != 17], clean.tendencies[:, torch.arange(300, device=dev) != 17])


def _round_to(ft, x):
    """The Fraction x rounded to nearest (ties to even) in the float type, as a Python float."""
    r = float(x)                                        # correctly rounded to double
    if ft == "f64":
        return r
    c = np.float32(r)                                   # a second rounding: right unless x sits between c and the true nearest neighbour
    best = min((np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))),
               key=lambda y: (abs(Fraction(float(y)) - x), int(np.float32(y).view(np.uint32)) & 1) if np.isfinite(y) else (Fraction(10) ** 60, 0))
    return float(best)


def _fma_chain(ft, g, d):
    """s = −0; s = fma(g_o, d_o, s) over the outputs, each step ONE rounding to the float type: what param_vjp_point forms per point and direction."""
    s = Fraction(0)
    for a, b in zip(g, d):
        s = Fraction(_round_to(ft, Fraction(float(a)) * Fraction(float(b)) + s))
    return float(s)


VJP_NAMES = ("SB2006_collection_kernel_coeff_kcc", "SB2006_rain_evaporation_coeff_beta", "condensation_evaporation_timescale")


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 262147])
def test_param_vjp_is_the_sum_of_the_jvp_columns(dev, ft, n):
    wr, tps = pc.params(ft, True, {})
    x = _states(n, ft, dev, seed=n)
    pairs = _pairs(wr, VJP_NAMES, False)
    S = cmx.warm_rain_param_jvp_2m(wr, tps, *x, pairs).jvp                      # [3, 4, n]
    gen = torch.Generator(device="cpu").manual_seed(n)
    g = [torch.randn(n, generator=gen, dtype=torch.float64).to(DT[ft]).to(dev) for _ in range(4)]
    S64, g64 = S.double().cpu().numpy(), [c.double().cpu().numpy() for c in g]
    u = 2.0 ** -53
    # one cotangent column at a time (the other members NULL): the device's terms are ḡ·S rounded once to the float type
    for o in range(4):
        cot = [g[q] if q == o else None for q in range(4)]
        v = cmx.warm_rain_param_vjp_2m(wr, tps, *x, cot, pairs)
        terms = (g[o][None] * S[:, o]).double().cpu().numpy()                   # the product in the float type, as the device forms it
        grad = v.grad.cpu().numpy()
        bound = 2 * n * u * np.abs(terms).sum(axis=1)
        assert (np.abs(grad - terms.sum(axis=1)) <= bound).all(), (ft, n, o, grad, terms.sum(axis=1), bound)
        assert _eq(cmx.warm_rain_param_vjp_2m(wr, tps, *x, cot, pairs).grad, v.grad)      # twice: the same bits
        assert _eq(cmx.warm_rain_param_vjp_2m(wr, tps, *x, cot, pairs[1:2]).grad, v.grad[1:2])      # alone: the same bits
    # all four: a chain of fused multiply-adds per point.  Up to 1025 points the chain is formed here exactly (rational arithmetic, rounded once per step
    # to the float type), so the bound is the issue's as it stands; at the largest size that is too slow for a test, and each term is known only to
    # (NOUT − 1)·eps(FT)·Σ_o |ḡ_o S_o|, which is added there and nowhere else (the strict bound is held at that size by the four calls above)
    v = cmx.warm_rain_param_vjp_2m(wr, tps, *x, g, pairs, with_tendencies=True)
    if n <= 1025:
        terms = np.array([[_fma_chain(ft, [g64[o][i] for o in range(4)], [S64[d, o, i] for o in range(4)]) for i in range(n)] for d in range(3)])
        bound = 2 * n * u * np.abs(terms).sum(axis=1)
    else:
        terms = sum(g64[o][None] * S64[:, o] for o in range(4))
        absum = sum(np.abs(g64[o][None] * S64[:, o]) for o in range(4)).sum(axis=1)
        bound = 2 * n * u * np.abs(terms).sum(axis=1) + 3 * float(np.finfo(NPT[ft]).eps) * absum
    assert (np.abs(v.grad.cpu().numpy() - terms.sum(axis=1)) <= bound).all(), (ft, n, v.grad, terms.sum(axis=1), bound)
    assert _eq(v.tendencies, _tendencies(wr, tps, x))
    # no cotangent at all: zeros
    assert not bool(cmx.warm_rain_param_vjp_2m(wr, tps, *x, [None] * 4, pairs).grad.any())


@pytest.mark.parametrize("ft", FTS)
def test_param_vjp_of_no_points_is_zero(dev, ft):
    wr, tps = pc.params(ft, True, {})
    x = [torch.empty(0, dtype=DT[ft], device=dev) for _ in range(7)]
    v = cmx.warm_rain_param_vjp_2m(wr, tps, *x, [torch.empty(0, dtype=DT[ft], device=dev)] * 4, VJP_NAMES)
    assert v.grad.shape == (3,) and not bool(v.grad.any()) and v.wrt == VJP_NAMES
    assert cmx.warm_rain_param_jvp_2m(wr, tps, *x, [{VJP_NAMES[0]: 1.0}]).jvp.shape == (1, 4, 0)


@pytest.mark.parametrize("ft", FTS)
def test_names_give_the_gradient_with_respect_to_the_parameter(dev, oracle, ft):
    """wrt = names: grad[k] = dL/dθ_k for L = Σ_i Σ_o ḡ_o,i·out_o,i, against the oracle's sensitivities: Σ ḡ·S^ref/θ within BOUND·Σ_i Σ_o |ḡ_o,i|·s_o,i/|θ_k|
    (the row measure summed over the kept states)."""
    cols, S_ref, kept, dead, _ = pc.reference(True, False, "interior")
    wr, tps = pc.params(ft, True, {})
    x = _dev_cols(cols, ft, dev)
    rng = np.random.default_rng(3)
    g = rng.standard_normal((4, cols[0].size)).astype(NPT[ft])
    g[:, ~kept] = 0                                                             # a state the reference set aside takes no part
    names = NO_EXPONENTS[:16]
    v = cmx.warm_rain_param_vjp_2m(wr, tps, *x, [torch.from_numpy(c).to(dev) for c in g], names)
    idx = [pc.NAMES.index(k) for k in names]
    th = pc.theta(False, names)
    ref = np.einsum("oi,opi->p", g.astype(np.float64), S_ref[:, idx]) / th
    s = np.abs(S_ref).max(axis=1)                                               # [4, n]: the row scale over all tested parameters
    bound = pc.BOUND[ft] * (np.abs(g.astype(np.float64)) * s).sum() / np.abs(th)
    got = v.grad.cpu().numpy()
    print(f"dL/dθ {ft}: worst fraction of the bound {np.max(np.abs(got - ref) / bound):.3g}")
    assert (np.abs(got - ref) <= bound).all(), (names, got, ref, bound)


@pytest.mark.parametrize("ft", FTS)
def test_both_entries_replay_from_a_graph(dev, ft):
    wr, tps = pc.params(ft, True, {})
    x = _states(4099, ft, dev)
    pairs = _pairs(wr, VJP_NAMES, False)
    g = [torch.ones_like(x[0]), None, torch.full_like(x[0], -2.0), None]
    jvp, tend = torch.empty((3, 4, 4099), dtype=DT[ft], device=dev), torch.empty((4, 4099), dtype=DT[ft], device=dev)
    eager_j = cmx.warm_rain_param_jvp_2m(wr, tps, *x, pairs, with_tendencies=True)
    eager_v = cmx.warm_rain_param_vjp_2m(wr, tps, *x, g, pairs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cmx.warm_rain_param_jvp_2m(wr, tps, *x, pairs, with_tendencies=True, out=(jvp, tend))
        cap_v = cmx.warm_rain_param_vjp_2m(wr, tps, *x, g, pairs)
    graph.replay()
    torch.cuda.synchronize()
    assert _eq(jvp, eager_j.jvp) and _eq(tend, eager_j.tendencies) and _eq(cap_v.grad, eager_v.grad)
    x[3].mul_(1.5)                                                              # new state in the captured columns: the replay follows it
    graph.replay()
    torch.cuda.synchronize()
    assert _eq(jvp, cmx.warm_rain_param_jvp_2m(wr, tps, *x, pairs).jvp) and _eq(cap_v.grad, cmx.warm_rain_param_vjp_2m(wr, tps, *x, g, pairs).grad)
    assert not _eq(cap_v.grad, eager_v.grad)


def test_wrapper_argument_errors(dev):
    wr, tps = pc.params("f32", True, {})
    x = _states(8, "f32", dev)
    with pytest.raises(ValueError):
        cmx.warm_rain_param_jvp_2m(wr, tps, *x, [])
    with pytest.raises(ValueError):
        cmx.warm_rain_param_jvp_2m(wr, tps, *x, [{"SB2006_raindrops_terminal_velocity_coeff_aR": 1.0}])
    with pytest.raises(TypeError):
        cmx.warm_rain_param_jvp_2m(wr, tps, *x, [P.parameter_direction(P.WarmRainParams2M("f64"), {"gas_constant_vapor": 1.0})])
    with pytest.raises(ValueError):
        cmx.warm_rain_param_vjp_2m(wr, tps, *x, [None] * 3, ["gas_constant_vapor"])
    bad = P.parameter_direction(wr, {"gas_constant_vapor": 1.0})
    bad[0].seifert_beheng.acnv.kcc = float("inf")
    with pytest.raises(cmx.CmxStatusError):
        cmx.warm_rain_param_jvp_2m(wr, tps, *x, [bad])
