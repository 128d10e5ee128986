"""The Python front of the products with the Jacobian without a GPU: the argument validation of cmx.warm_rain_jvp_2m / warm_rain_vjp_2m / jvp_1m / vjp_1m
(every error below is raised before any device is touched), the rho errors of cmx.autograd, and the rules of the autograd layer itself — which inputs are
requested from the VJP launch, None gradients and tangents, contiguous cotangents, no launch without a cotangent, once-differentiable — on a stand-in scheme
whose three launches are plain torch on the CPU (cmx.autograd._function is the factory both real schemes are made with; tests/test_autograd_gpu.py runs
those on the device)."""
from collections import namedtuple

import pytest
import torch
import torch.autograd.forward_ad as fwAD

import cmx
from cmx import _abi
from cmx import autograd as A
from cmx import parameters as P

F64 = torch.float64


def _cols(n=4):
    return [torch.ones(n, dtype=F64) for _ in range(7)]


PRODUCTS = [("sb2006", lambda ft: P.WarmRainParams2M(ft, True), cmx.warm_rain_jvp_2m, cmx.warm_rain_vjp_2m, cmx.JACOBIAN_WRT, "n_lcl", "q_icl"),
            ("mp1m", lambda ft: P.Microphysics1MParams(ft), cmx.jvp_1m, cmx.vjp_1m, cmx.JACOBIAN_WRT_1M, "q_icl", "n_lcl")]


@pytest.mark.parametrize("name,params,jvp,vjp,wrt,own,foreign", PRODUCTS, ids=[p[0] for p in PRODUCTS])
def test_product_functions_validate_their_arguments(name, params, jvp, vjp, wrt, own, foreign):
    mp, tps = params("f64"), P.ThermodynamicsParameters("f64")
    cols, one = _cols(), torch.ones(4, dtype=F64)
    # tangents: a dict over the differentiable inputs
    with pytest.raises(TypeError, match="tangents must be a dict"):
        jvp(mp, tps, *cols, [one] * 6)
    with pytest.raises(ValueError, match="rho is not differentiated"):
        jvp(mp, tps, *cols, {"rho": one})
    with pytest.raises(ValueError, match=f"unknown input '{foreign}'"):
        jvp(mp, tps, *cols, {foreign: one})
    # wrt: names, once each; rho is not among them
    with pytest.raises(ValueError, match="rho is not differentiated"):
        vjp(mp, tps, *cols, [one] * 4, wrt=("T", "rho"))
    with pytest.raises(ValueError, match=f"unknown input '{foreign}'"):
        vjp(mp, tps, *cols, [one] * 4, wrt=(foreign,))
    with pytest.raises(ValueError, match="listed twice"):
        vjp(mp, tps, *cols, [one] * 4, wrt=(own, own))
    with pytest.raises(ValueError, match="nothing to compute"):
        vjp(mp, tps, *cols, [one] * 4, wrt=())
    with pytest.raises(ValueError, match="4 tensors"):
        vjp(mp, tps, *cols, [one] * 3)
    # parameters and columns
    with pytest.raises(TypeError, match="mp must be"):
        jvp(object(), tps, *cols, {})
    with pytest.raises(TypeError, match="mp must be"):
        vjp(object(), tps, *cols, [None] * 4)
    for call in (lambda: jvp(mp, tps, *cols, {own: one}), lambda: vjp(mp, tps, *cols, [one] * 4)):
        with pytest.raises(ValueError, match="resident on the GPU"):          # there is no CPU path
            call()
    assert tuple(wrt) == (_abi.SB2006_JAC_WRT if name == "sb2006" else _abi.MP1M_JAC_WRT)


def test_result_types_are_exported():
    assert cmx.WarmRainJvp2M._fields == cmx.Jvp1M._fields == ("jvp", "tendencies")
    assert cmx.WarmRainVjp2M._fields == cmx.Vjp1M._fields == ("grad", "tendencies", "wrt")
    assert set(A.__all__) == {"warm_rain_tendencies_2m", "tendencies_1m"}
    for stem in _abi.JACOBIAN_PRODUCT_STEMS:
        for product in ("jvp", "vjp"):
            for ft in ("f32", "f64"):
                assert hasattr(cmx._lib.lib(), f"{stem}_{product}_{ft}")


@pytest.mark.parametrize("fn,params", [(A.warm_rain_tendencies_2m, lambda: P.WarmRainParams2M("f64", True)), (A.tendencies_1m, lambda: P.Microphysics1MParams("f64"))],
                         ids=["sb2006", "mp1m"])
def test_rho_is_not_differentiated(fn, params):
    """rho.requires_grad and a forward-mode tangent on rho raise at the call, before any device is touched (the columns here live on the CPU)."""
    mp, tps = params(), P.ThermodynamicsParameters("f64")
    cols = _cols()
    cols[0].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="rho"):
        fn(mp, tps, *cols)
    cols[0] = cols[0].detach()
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError, match="rho"):
            fn(mp, tps, fwAD.make_dual(cols[0], torch.ones(4, dtype=F64)), *cols[1:])


# ---- the rules of the autograd layer on a stand-in scheme ----------------------------------------------------------------------------------------
# out_o = Σ_j M[o, j]·x_j² over three differentiable inputs a, b, c (rho: column 0, held fixed): J_oj = 2 M[o, j] x_j
M = torch.tensor([[1.0, 2.0, 0.0], [0.0, 3.0, 1.0], [2.0, 0.0, 5.0], [1.0, 1.0, 1.0]], dtype=F64)
WRT = ("a", "b", "c")
Grad = namedtuple("Grad", ["grad", "wrt"])
Jvp = namedtuple("Jvp", ["jvp"])


@pytest.fixture
def toy():
    calls = []

    def primal(mp, tps, cols):
        return [sum(M[o, j] * cols[1 + j] ** 2 for j in range(3)) for o in range(4)]

    def vjp(mp, tps, cols, cotangents, wrt):
        calls.append(("vjp", wrt, [None if g is None else (g.is_contiguous(), g.stride()) for g in cotangents]))
        assert all(g is None or g.is_contiguous() for g in cotangents)
        return Grad(torch.stack([sum(cotangents[o] * 2 * M[o, WRT.index(n)] * cols[1 + WRT.index(n)] for o in range(4) if cotangents[o] is not None)
                                 + torch.zeros_like(cols[0]) for n in wrt]), wrt)

    def jvp(mp, tps, cols, tangents):
        calls.append(("jvp", tuple(tangents), None))
        return Jvp(torch.stack([sum((2 * M[o, WRT.index(n)] * cols[1 + WRT.index(n)] * t for n, t in tangents.items()), torch.zeros_like(cols[0])) for o in range(4)]))
    return A._function("Toy", WRT, primal, vjp, jvp), calls


def _state(requires=(True, True, True)):
    g = torch.Generator().manual_seed(1)
    cols = [torch.rand(5, dtype=F64, generator=g) + 0.5 for _ in range(4)]
    for c, r in zip(cols[1:], requires):
        c.requires_grad_(r)
    return cols


def test_backward_requests_only_what_is_needed(toy):
    F, calls = toy
    cols = _state((True, False, True))
    out = F.apply("mp", "tps", *cols)
    w = [torch.full((5,), float(k + 1), dtype=F64) for k in range(4)]
    ga, gc = torch.autograd.grad(sum((wk * o).sum() for wk, o in zip(w, out)), [cols[1], cols[3]])
    assert calls == [("vjp", ("a", "c"), [(True, (1,))] * 4)]          # one launch, for the two inputs that need a gradient
    J = 2 * M[:, :, None] * torch.stack(cols[1:])[None].detach()
    want = torch.einsum("ojn,on->jn", J, torch.stack(w))
    assert torch.equal(ga, want[0]) and torch.equal(gc, want[2])


def test_outputs_outside_the_loss_are_null_cotangents_and_a_bare_sum_is_made_contiguous(toy):
    F, calls = toy
    cols = _state()
    out = F.apply("mp", "tps", *cols)
    (out[1].sum() + out[3].sum()).backward()          # the gradient of .sum() is a stride-0 expansion
    (kind, wrt, cot), = calls
    assert kind == "vjp" and wrt == WRT and cot[0] is None and cot[2] is None and cot[1] == cot[3] == (True, (1,))
    J = 2 * M[:, :, None] * torch.stack(cols[1:])[None].detach()
    assert torch.equal(torch.stack([c.grad for c in cols[1:]]), J[1] + J[3])
    assert cols[0].grad is None


def test_no_cotangent_or_no_input_means_no_launch(toy):
    F, calls = toy
    cols = _state((False, False, False))
    out = F.apply("mp", "tps", *cols)
    assert not any(o.requires_grad for o in out) and calls == []
    cols = _state()
    out = F.apply("mp", "tps", *cols)
    g = torch.autograd.grad(out[0].sum() * 0 + cols[1].sum(), cols[1:], allow_unused=True)        # the outputs reach the loss with a gradient …
    assert len(calls) == 1
    calls.clear()
    out = F.apply("mp", "tps", *cols)
    g = torch.autograd.grad(cols[1].sum(), cols[1:], allow_unused=True)                           # … or not at all
    assert calls == [] and g[1] is None


def test_backward_is_once_differentiable(toy):
    F, _ = toy
    cols = _state()
    out = F.apply("mp", "tps", *cols)
    w = torch.ones(5, dtype=F64, requires_grad=True)          # a cotangent that is itself part of a graph: the gradient then carries torch's error node
    g, = torch.autograd.grad((w * out[0]).sum(), cols[1], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_forward_mode_passes_missing_tangents_as_missing(toy):
    F, calls = toy
    cols = _state((False, False, False))
    ta, tc = torch.full((5,), 2.0, dtype=F64), torch.full((5,), -1.0, dtype=F64)
    with fwAD.dual_level():
        out = F.apply("mp", "tps", cols[0], fwAD.make_dual(cols[1], ta), cols[2], fwAD.make_dual(cols[3], tc))
        tangents = [fwAD.unpack_dual(o).tangent for o in out]
    assert calls == [("jvp", ("a", "c"), None)]
    J = 2 * M[:, :, None] * torch.stack(cols[1:])[None]
    assert torch.equal(torch.stack(tangents), J[:, 0] * ta + J[:, 2] * tc)
