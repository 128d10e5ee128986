"""torch autograd through the tendencies on the device (cmx.autograd.warm_rain_tendencies_2m, cmx.autograd.tendencies_1m): the forward pass against the plain
entries, reverse mode against the fused Jᵀḡ entry called directly and forward mode against the fused J v entry, all bit for bit — the autograd layer adds no
arithmetic of its own — on 257 interior states, both schemes, both float types.  (That the products themselves are right is tests/test_jacobian_products_gpu.py;
the rules of the layer on a stand-in scheme without a GPU are tests/test_autograd_host.py.)"""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import jacobian_products_cases as PC
from jacobian_products_cases import SCHEMES
import cmx
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
N = 257


def _plain_2m(mp, tps, cols):
    return list(cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), mp, tps, *cols))[:4]


def _plain_1m(mp, tps, cols):
    return list(cmx.bulk_microphysics_tendencies_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), mp, tps, *cols))


API = {"sb2006": (cmx.autograd.warm_rain_tendencies_2m, _plain_2m, cmx.warm_rain_vjp_2m, cmx.warm_rain_jvp_2m),
       "mp1m": (cmx.autograd.tendencies_1m, _plain_1m, cmx.vjp_1m, cmx.jvp_1m)}
PARAMS = [(n, ft) for n in ("sb2006", "mp1m") for ft in ("f64", "f32")]


def _eq(a, b):
    """Same bits, NaN = NaN."""
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


@pytest.fixture(scope="module", params=PARAMS, ids=[f"{n}-{ft}" for n, ft in PARAMS])
def setup(request, oracle):
    name, ft = request.param
    scheme = SCHEMES[name]
    case, which = scheme.INTERIOR
    ref_cols, J_ref, _, _ = scheme.reference(case, which)
    dev = torch.device("cuda:0")
    to = lambda cs: [torch.from_numpy(np.array(c[:N], dtype=np.float64)).to(DT[ft]).to(dev) for c in cs]  # noqa: E731
    _, v, g, *_ = PC.mixed_vectors([c[:N] for c in ref_cols], J_ref[:, :, :N])
    return scheme, API[name], scheme.params(ft, case), P.ThermodynamicsParameters(ft), to(ref_cols), to(v), to(g)


def _leaves(cols, requires):
    return [cols[0]] + [c.clone().requires_grad_(r) for c, r in zip(cols[1:], requires)]


def test_forward_is_the_plain_entry_bit_for_bit(setup):
    scheme, (fn, plain, _, _), mp, tps, cols, _, _ = setup
    want = plain(mp, tps, cols)
    for requires in ([False] * 6, [True] * 6):
        out = fn(mp, tps, *_leaves(cols, requires))
        assert len(out) == 4 and all(_eq(o.detach(), w) for o, w in zip(out, want))
        assert all(o.requires_grad == requires[0] for o in out)


def test_grad_is_the_vjp_entry_bit_for_bit(setup):
    """torch.autograd.grad of Σ_q (w_q·out_q).sum() — all inputs, some inputs, some outputs (None cotangents), and a bare .sum() (a stride-0 gradient)."""
    scheme, (fn, _, vjp, _), mp, tps, cols, _, w = setup
    # every input, every output
    x = _leaves(cols, [True] * 6)
    grads = torch.autograd.grad(sum((wq * o).sum() for wq, o in zip(w, fn(mp, tps, *x))), x[1:])
    direct = vjp(mp, tps, *cols, w).grad
    assert all(_eq(g, d) for g, d in zip(grads, direct))
    # only some inputs require grad: the others get no gradient, the requested ones the same bits
    requires = [True, False, False, True, True, False]
    x = _leaves(cols, requires)
    sub = [t for t, r in zip(x[1:], requires) if r]
    grads = torch.autograd.grad(sum((wq * o).sum() for wq, o in zip(w, fn(mp, tps, *x))), sub)
    wrt = tuple(n for n, r in zip(scheme.WRT, requires) if r)
    assert all(_eq(g, d) for g, d in zip(grads, vjp(mp, tps, *cols, w, wrt=wrt).grad))
    assert all(_eq(g, direct[scheme.WRT.index(n)]) for g, n in zip(grads, wrt))
    # only some outputs enter the loss: None cotangents, not zeros
    x = _leaves(cols, [True] * 6)
    out = fn(mp, tps, *x)
    grads = torch.autograd.grad((w[1] * out[1]).sum() + (w[3] * out[3]).sum(), x[1:])
    assert all(_eq(g, d) for g, d in zip(grads, vjp(mp, tps, *cols, [None, w[1], None, w[3]]).grad))
    # a bare .sum(): the incoming gradient is a stride-0 expansion of a scalar one
    x = _leaves(cols, [True] * 6)
    fn(mp, tps, *x)[2].sum().backward()
    one = torch.ones_like(cols[0])
    assert all(_eq(t.grad, d) for t, d in zip(x[1:], vjp(mp, tps, *cols, [None, None, one, None]).grad))
    assert x[0].grad is None


def test_forward_mode_is_the_jvp_entry_bit_for_bit(setup):
    scheme, (fn, plain, _, jvp), mp, tps, cols, v, _ = setup
    want = plain(mp, tps, cols)
    for given in (list(range(6)), [0, 4]):
        with fwAD.dual_level():
            x = [cols[0]] + [fwAD.make_dual(c, v[j]) if j in given else c for j, c in enumerate(cols[1:])]
            out = [fwAD.unpack_dual(o) for o in fn(mp, tps, *x)]
        direct = jvp(mp, tps, *cols, {scheme.WRT[j]: v[j] for j in given}).jvp
        assert all(_eq(o.primal, p) for o, p in zip(out, want))
        assert all(_eq(o.tangent, d) for o, d in zip(out, direct)), given


def test_rho_requires_grad_raises(setup):
    scheme, (fn, _, _, _), mp, tps, cols, v, _ = setup
    with pytest.raises(NotImplementedError, match="rho"):
        fn(mp, tps, cols[0].clone().requires_grad_(True), *cols[1:])
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError, match="rho"):
            fn(mp, tps, fwAD.make_dual(cols[0], v[0]), *cols[1:])


def test_a_second_backward_raises(setup):
    scheme, (fn, _, _, _), mp, tps, cols, _, w = setup
    x = _leaves(cols, [True] * 6)
    w0 = w[0].clone().requires_grad_(True)          # a cotangent that is itself part of a graph: the gradient then carries torch's error node
    g, = torch.autograd.grad((w0 * fn(mp, tps, *x)[0]).sum(), x[1], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
