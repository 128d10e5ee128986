"""`cmx.autograd.warm_rain_tendencies_2m(…, theta=, names=)` on the device: `loss.backward()` fills `theta.grad` through cmx_sb2006_warm_rain_param_vjp_*
(include/cmx.h §22), checked against the oracle's central differences (tests/param_cases.py: Σ ḡ·S^ref/θ within BOUND·Σ_i Σ_o |ḡ_o,i|·s_o,i/|θ_p|, the row
measure summed over the kept states); the forward pass and the state gradients are those of the function without `theta`, bit for bit; forward mode with a
tangent on `theta` is the param_jvp entry; a `theta` that is not a 1-D CPU float64 tensor is a TypeError."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import param_cases as pc
import cmx
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
NAMES = tuple(k for k in pc.NAMES if k not in pc.EXPONENTS)[:12] + ("gas_constant_vapor",)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _cols(cols, ft, dev, requires_grad=False):
    x = [torch.from_numpy(np.array(c, dtype=np.float64)).to(DT[ft]).to(dev) for c in cols]
    for t in x[1:]:
        t.requires_grad_(requires_grad)
    return x


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_backward_fills_theta_grad(dev, oracle, ft):
    cols, S_ref, kept, dead, _ = pc.reference(True, False, "interior")
    wr, tps = pc.params(ft, True, {})
    x = _cols(cols, ft, dev)
    th = pc.theta(False, NAMES)
    theta = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    rng = np.random.default_rng(9)
    g = rng.standard_normal((4, cols[0].size))
    g[:, ~kept] = 0
    w = torch.from_numpy(g).to(DT[ft]).to(dev)
    out = cmx.autograd.warm_rain_tendencies_2m(wr, tps, *x, theta=theta, names=NAMES)
    plain = cmx.autograd.warm_rain_tendencies_2m(wr, tps, *x)
    assert all(torch.equal(a, b) for a, b in zip(out, plain))                   # theta holds the defaults: the same structs, the same entry
    sum((w[o] * out[o]).sum() for o in range(4)).backward()
    assert theta.grad is not None and theta.grad.dtype == torch.float64 and theta.grad.device.type == "cpu" and theta.grad.shape == theta.shape
    idx = [pc.NAMES.index(k) for k in NAMES]
    gq = w.double().cpu().numpy()                                               # the cotangents as the device read them
    ref = np.einsum("oi,opi->p", gq, S_ref[:, idx]) / th
    bound = pc.BOUND[ft] * (np.abs(gq) * np.abs(S_ref).max(axis=1)).sum() / np.abs(th)
    got = theta.grad.numpy()
    print(f"theta.grad {ft}: worst fraction of the bound {np.max(np.abs(got - ref) / bound):.3g}")
    assert (np.abs(got - ref) <= bound).all(), (got, ref, bound)


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_state_gradients_are_those_of_the_function_without_theta(dev, ft):
    cols = [c[:1025] for c in pc.states("interior")]
    wr, tps = pc.params(ft, True, {})
    theta = torch.tensor(pc.theta(False, NAMES), dtype=torch.float64, requires_grad=True)
    grads = []
    for kw in (dict(theta=theta, names=NAMES), {}):
        x = _cols(cols, ft, dev, requires_grad=True)
        out = cmx.autograd.warm_rain_tendencies_2m(wr, tps, *x, **kw)
        (out[0].sum() - 3 * out[2].sum() + (out[3] * x[1].detach()).sum()).backward()      # dn_lcl_dt does not enter the loss: a NULL cotangent
        grads.append([t.grad for t in x[1:]])
    assert all(a is not None and torch.equal(a, b) for a, b in zip(*grads))
    assert theta.grad is not None and bool(torch.isfinite(theta.grad).all())
    # theta alone: no state launch is needed, and the values move the forward pass
    x = _cols(cols, ft, dev)
    moved = cmx.autograd.warm_rain_tendencies_2m(wr, tps, *x, theta=theta.detach() * 1.1, names=NAMES)
    assert not torch.equal(moved[0], cmx.autograd.warm_rain_tendencies_2m(wr, tps, *x)[0])


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_forward_mode_with_a_tangent_on_theta(dev, ft):
    cols = [c[:300] for c in pc.states("interior")]
    wr, tps = pc.params(ft, True, {})
    x = _cols(cols, ft, dev)
    th = torch.tensor(pc.theta(False, NAMES), dtype=torch.float64)
    t = torch.linspace(-1.0, 1.0, len(NAMES), dtype=torch.float64) * th
    with fwAD.dual_level():
        out = cmx.autograd.warm_rain_tendencies_2m(wr, tps, *x, theta=fwAD.make_dual(th, t), names=NAMES)
        tangents = [fwAD.unpack_dual(o).tangent for o in out]
    ref = cmx.warm_rain_param_jvp_2m(wr, tps, *x, [dict(zip(NAMES, t.tolist()))]).jvp[0]
    assert all(torch.equal(a, ref[o]) for o, a in enumerate(tangents))


def test_theta_must_be_a_cpu_float64_vector(dev):
    wr, tps = pc.params("f32", True, {})
    x = _cols([c[:8] for c in pc.states("interior")], "f32", dev)
    th = torch.tensor(pc.theta(False, NAMES), dtype=torch.float64)
    for bad in (th.float(), th.to(dev), th[None], th.tolist()):
        with pytest.raises(TypeError):
            cmx.autograd.warm_rain_tendencies_2m(wr, tps, *x, theta=bad, names=NAMES)
    with pytest.raises(ValueError):
        cmx.autograd.warm_rain_tendencies_2m(wr, tps, *x, theta=th, names=NAMES[:-1])
    with pytest.raises(ValueError):
        cmx.autograd.warm_rain_tendencies_2m(wr, tps, *x, theta=th[:1], names=["SB2006_raindrops_terminal_velocity_coeff_aR"])
    with pytest.raises(ValueError):
        cmx.autograd.warm_rain_tendencies_2m(wr, tps, *x, names=NAMES)
    # the forward pass rebuilds the structs from mp's dictionary: a field edited after construction would be lost, so it is refused
    edited, _ = pc.params("f32", True, {})
    edited.c.seifert_beheng.acnv.kcc *= 2
    with pytest.raises(ValueError):
        cmx.autograd.warm_rain_tendencies_2m(edited, tps, *x, theta=th, names=NAMES)
    tps2 = type(tps).from_buffer_copy(tps)
    tps2.cp_l *= 1.01
    with pytest.raises(ValueError):
        cmx.autograd.warm_rain_tendencies_2m(wr, tps2, *x, theta=th, names=NAMES)                     # NAMES holds a thermodynamics name
    out = cmx.autograd.warm_rain_tendencies_2m(wr, tps2, *x, theta=th[:1], names=NAMES[:1])            # no thermodynamics name: tps is used as it is
    assert torch.equal(out[0], cmx.autograd.warm_rain_tendencies_2m(wr, tps2, *x)[0])
    # overrides given through the dictionary survive the rebuild
    ov, _ = pc.params("f32", True, {"SB2006_collection_kernel_coeff_kcr": 6.0})
    out = cmx.autograd.warm_rain_tendencies_2m(ov, tps, *x, theta=th[:1], names=NAMES[:1])
    assert torch.equal(out[2], cmx.autograd.warm_rain_tendencies_2m(ov, tps, *x)[2])
