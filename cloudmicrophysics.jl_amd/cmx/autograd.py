"""torch autograd for the tendencies: `cmx.autograd.warm_rain_tendencies_2m` and `cmx.autograd.tendencies_1m` compute what
`cmx.bulk_microphysics_tendencies` / `cmx.bulk_microphysics_tendencies_1m(Instantaneous(), …)` compute — the forward pass IS that entry, bit for bit — and
can be differentiated by `loss.backward()`, `torch.autograd.grad` and `torch.autograd.forward_ad`:

  * backward calls the fused Jᵀḡ entry (`warm_rain_vjp_2m` / `vjp_1m`) ONCE, for exactly the inputs that need a gradient; an output that does not enter the
    loss (a `None` gradient) is a NULL cotangent; if no output enters it, nothing is launched;
  * forward mode calls the fused J v entry (`warm_rain_jvp_2m` / `jvp_1m`); an input without a tangent is a NULL tangent column.

ρ is held fixed by the Jacobian entries, so `rho.requires_grad`, or a forward-mode tangent on `rho`, raises NotImplementedError at the call: a silently missing
gradient is worse than an error.  Not built: double backward (backward is once-differentiable), vmap, the derivative with respect to the parameters, the
fall-speed outputs, LinearizedAverage and the 2M + P3 scheme."""
import torch
from torch.autograd.function import once_differentiable

from . import bulk_tendencies as _bt
from . import microphysics1m as _m1

__all__ = ["warm_rain_tendencies_2m", "tendencies_1m"]


def _check_rho(rho):
    if rho.requires_grad:
        raise NotImplementedError("rho.requires_grad: the air density is held fixed, the tendencies are not differentiated with respect to rho")
    if torch.autograd.forward_ad.unpack_dual(rho).tangent is not None:
        raise NotImplementedError("forward-mode tangent on rho: the air density is held fixed, the tendencies are not differentiated with respect to rho")


def _function(name, WRT, primal, vjp, jvp):
    """The torch.autograd.Function of one scheme: WRT names the differentiable inputs (state columns 1 … 6), the three callables are its launches."""
    class F(torch.autograd.Function):
        @staticmethod
        def forward(mp, tps, *cols):
            return tuple(primal(mp, tps, cols))

        @staticmethod
        def setup_context(ctx, inputs, output):
            mp, tps, *cols = inputs
            ctx.mp, ctx.tps = mp, tps
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(*cols)
            ctx.save_for_forward(*cols)

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            wrt = tuple(n for k, n in enumerate(WRT) if ctx.needs_input_grad[3 + k])
            out = [None] * (3 + len(WRT))            # mp, tps, rho, then the differentiable inputs
            if not wrt or all(g is None for g in grads):
                return tuple(out)
            # the gradient of out.sum() arrives as a stride-0 expansion: the entry reads columns
            r = vjp(ctx.mp, ctx.tps, ctx.saved_tensors, [g.contiguous() if g is not None else None for g in grads], wrt)
            for k, n in enumerate(wrt):
                out[3 + WRT.index(n)] = r.grad[k]
            return tuple(out)

        @staticmethod
        def jvp(ctx, t_mp, t_tps, t_rho, *tangents):
            if t_rho is not None:
                raise NotImplementedError("forward-mode tangent on rho: the air density is held fixed")
            r = jvp(ctx.mp, ctx.tps, ctx.saved_tensors, {n: t.contiguous() for n, t in zip(WRT, tangents) if t is not None})
            return tuple(r.jvp[o] for o in range(4))
    F.__name__ = F.__qualname__ = name
    return F


_WarmRain2M = _function(
    "WarmRainTendencies2M", _bt.JACOBIAN_WRT,
    lambda mp, tps, cols: _bt.bulk_microphysics_tendencies(_bt.Microphysics2Moment(), mp, tps, *cols)[:4],
    lambda mp, tps, cols, cotangents, wrt: _bt.warm_rain_vjp_2m(mp, tps, *cols, cotangents, wrt=wrt),
    lambda mp, tps, cols, tangents: _bt.warm_rain_jvp_2m(mp, tps, *cols, tangents))

_Tendencies1M = _function(
    "Tendencies1M", _m1.JACOBIAN_WRT_1M,
    lambda mp, tps, cols: _m1.bulk_microphysics_tendencies_1m(_m1.Instantaneous(), _m1.Microphysics1Moment(), mp, tps, *cols),
    lambda mp, tps, cols, cotangents, wrt: _m1.vjp_1m(mp, tps, *cols, cotangents, wrt=wrt),
    lambda mp, tps, cols, tangents: _m1.jvp_1m(mp, tps, *cols, tangents))


def warm_rain_tendencies_2m(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai):
    """(dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt) of `cmx.bulk_microphysics_tendencies(Microphysics2Moment(), mp, tps, …)`, bit for bit, differentiable by
    torch with respect to T, q_tot, q_lcl, n_lcl, q_rai, n_rai (reverse and forward mode; module docstring)."""
    _check_rho(rho)
    return _WarmRain2M.apply(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)


def tendencies_1m(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno):
    """(dq_lcl_dt, dq_icl_dt, dq_rai_dt, dq_sno_dt) of `cmx.bulk_microphysics_tendencies_1m(Instantaneous(), Microphysics1Moment(), mp, tps, …)`, bit for bit,
    differentiable by torch with respect to T, q_tot, q_lcl, q_icl, q_rai, q_sno (reverse and forward mode; module docstring).  Instantaneous mode only."""
    _check_rho(rho)
    return _Tendencies1M.apply(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
