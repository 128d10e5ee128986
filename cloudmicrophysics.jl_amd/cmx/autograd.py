"""torch autograd for the tendencies: `cmx.autograd.warm_rain_tendencies_2m` and `cmx.autograd.tendencies_1m` compute what
`cmx.bulk_microphysics_tendencies` / `cmx.bulk_microphysics_tendencies_1m(Instantaneous(), …)` compute — the forward pass IS that entry, bit for bit — and
can be differentiated by `loss.backward()`, `torch.autograd.grad` and `torch.autograd.forward_ad`:

  * backward calls the fused Jᵀḡ entry (`warm_rain_vjp_2m` / `vjp_1m`) ONCE, for exactly the inputs that need a gradient; an output that does not enter the
    loss (a `None` gradient) is a NULL cotangent; if no output enters it, nothing is launched;
  * forward mode calls the fused J v entry (`warm_rain_jvp_2m` / `jvp_1m`); an input without a tangent is a NULL tangent column.

ρ is held fixed by the Jacobian entries, so `rho.requires_grad`, or a forward-mode tangent on `rho`, raises NotImplementedError at the call: a silently missing
gradient is worse than an error.  `warm_rain_tendencies_2m(…, theta=, names=)` and `tendencies_1m(…, theta=, names=)` also differentiate with respect to the scheme's PARAMETERS: `theta` is a 1-D CPU float64 tensor holding the
values of the ClimaParams `names`; the forward pass rebuilds the parameter structs with those values (host work, no device sync) and is otherwise the same
entry; backward calls the parameter-gradient entry (`warm_rain_param_vjp_2m` / `param_vjp_1m`) once for `theta.grad` (and the state Jᵀḡ entry if a state column needs a gradient), forward mode with a tangent on
`theta` calls `warm_rain_param_jvp_2m` / `param_jvp_1m`.  `cmx.autograd.column_tendencies_sedimentation_2m` is the SB2006 column step with sedimentation and its precipitation flux (`cmx.column_tendencies_sedimentation`),
differentiated through the fall speeds and the flux divergence by `column_vjp_2m` / `column_jvp_2m`; ρ and `inv_dz` are held fixed.  `cmx.autograd.column_tendencies_sedimentation_1m` is the same for the 1-moment column step
(`cmx.column_tendencies_sedimentation_1m`, Instantaneous mode) with its two precipitation fluxes, by `column_vjp_1m` / `column_jvp_1m`.  Not built: double backward (backward is once-differentiable), vmap, the
fall-speed outputs of the pointwise entry, LinearizedAverage and the 2M + P3 scheme.  With `theta=, names=` the column step is also differentiated with respect to the
parameters, the fall-speed parameters included (`column_param_vjp_2m` / `column_param_jvp_2m`, include/cmx.h §26; the 1-moment column step:
`column_param_vjp_1m` / `column_param_jvp_1m`, §28)."""
import torch
from torch.autograd.function import once_differentiable

from . import bulk_tendencies as _bt
from . import microphysics1m as _m1
from . import parameters as _P

__all__ = ["warm_rain_tendencies_2m", "tendencies_1m"]      # (tests/test_autograd_host.py pins the pointwise pair; the column step is reached by its name)


def _check_rho(rho):
    if rho.requires_grad:
        raise NotImplementedError("rho.requires_grad: the air density is held fixed, the tendencies are not differentiated with respect to rho")
    if torch.autograd.forward_ad.unpack_dual(rho).tangent is not None:
        raise NotImplementedError("forward-mode tangent on rho: the air density is held fixed, the tendencies are not differentiated with respect to rho")


def _function(name, WRT, primal, vjp, jvp, tangents_out=lambda r: tuple(r.jvp[o] for o in range(4))):
    """The torch.autograd.Function of one scheme: WRT names the differentiable inputs (state columns 1 … 6), the three callables are its launches;
    tangents_out: the output tangents from what `jvp` returns (an entry with more than the four point outputs gives its own)."""
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
            return tangents_out(r)
    F.__name__ = F.__qualname__ = name
    return F


_WarmRain2M = _function(
    "WarmRainTendencies2M", _bt.JACOBIAN_WRT,
    lambda mp, tps, cols: _bt.bulk_microphysics_tendencies(_bt.Microphysics2Moment(), mp, tps, *cols)[:4],
    lambda mp, tps, cols, cotangents, wrt: _bt.warm_rain_vjp_2m(mp, tps, *cols, cotangents, wrt=wrt),
    lambda mp, tps, cols, tangents: _bt.warm_rain_jvp_2m(mp, tps, *cols, tangents))


class _ColumnStep:
    """What the column step takes next to the parameters and the state — held fixed, not differentiated: travels in the `mp` slot of `_function`."""
    def __init__(self, mp, inv_dz, options):
        self.mp, self.inv_dz, self.options = mp, inv_dz, options


def _column_primal(step, tps, cols):
    r = _bt.column_tendencies_sedimentation(step.mp, tps, step.inv_dz, *cols, want_precip_flux=True, **step.options)
    return tuple(r)


# five outputs: the four tendencies and the precipitation flux (one value per column); its cotangent is the fifth gradient
_Column2M = _function(
    "ColumnTendenciesSedimentation2M", _bt.JACOBIAN_WRT, _column_primal,
    lambda step, tps, cols, cotangents, wrt: _bt.column_vjp_2m(step.mp, tps, step.inv_dz, *cols, cotangents[:4], cotangents[4], wrt=wrt, **step.options),
    lambda step, tps, cols, tangents: _bt.column_jvp_2m(step.mp, tps, step.inv_dz, *cols, tangents, **step.options),
    tangents_out=lambda r: (*(r.jvp[o] for o in range(4)), r.jvp_precip))

# the 1-moment column step: `step.mp` holds (mp, stokes, chen_rain, chen_ice); six outputs — the four tendencies and the two precipitation fluxes
_Column1M = _function(
    "ColumnTendenciesSedimentation1M", _m1.JACOBIAN_WRT_1M,
    lambda step, tps, cols: tuple(_m1.column_tendencies_sedimentation_1m(_m1.Instantaneous(), _m1.Microphysics1Moment(), step.mp[0], tps, *step.mp[1:],
                                                                          step.inv_dz, *cols)),
    lambda step, tps, cols, cotangents, wrt: _m1.column_vjp_1m(step.mp[0], tps, *step.mp[1:], step.inv_dz, *cols, cotangents[:4], cotangents[4], cotangents[5],
                                                                wrt=wrt),
    lambda step, tps, cols, tangents: _m1.column_jvp_1m(step.mp[0], tps, *step.mp[1:], step.inv_dz, *cols, tangents),
    tangents_out=lambda r: (*(r.jvp[o] for o in range(4)), r.jvp_precip_rai, r.jvp_precip_sno))

_Tendencies1M = _function(
    "Tendencies1M", _m1.JACOBIAN_WRT_1M,
    lambda mp, tps, cols: _m1.bulk_microphysics_tendencies_1m(_m1.Instantaneous(), _m1.Microphysics1Moment(), mp, tps, *cols),
    lambda mp, tps, cols, cotangents, wrt: _m1.vjp_1m(mp, tps, *cols, cotangents, wrt=wrt),
    lambda mp, tps, cols, tangents: _m1.jvp_1m(mp, tps, *cols, tangents))


def _theta_function(name, WRT, primal, vjp, jvp, param_vjp, param_jvp, tangents_out=lambda r: tuple(r.jvp[o] for o in range(4)),
                    param_tangents_out=lambda r: tuple(r.jvp[0][o] for o in range(4))):
    """The torch.autograd.Function of one scheme as a function of the parameter values `theta` (CPU) and the state: inputs (mp, tps, names, theta, rho, six
    columns), where mp / tps are the parameter objects already rebuilt with `theta`."""
    class F(torch.autograd.Function):
        @staticmethod
        def forward(mp, tps, names, theta, *cols):
            return tuple(primal(mp, tps, cols))

        @staticmethod
        def setup_context(ctx, inputs, output):
            ctx.mp, ctx.tps, ctx.names, _, *cols = inputs
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(*cols)
            ctx.save_for_forward(*cols)

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            out = [None] * (5 + len(WRT))                # mp, tps, names, theta, rho, then the differentiable inputs
            if all(g is None for g in grads):
                return tuple(out)
            cot = [g.contiguous() if g is not None else None for g in grads]
            if ctx.needs_input_grad[3]:
                out[3] = param_vjp(ctx.mp, ctx.tps, ctx.saved_tensors, cot, ctx.names).grad.cpu()
            wrt = tuple(n for k, n in enumerate(WRT) if ctx.needs_input_grad[5 + k])
            if wrt:
                r = vjp(ctx.mp, ctx.tps, ctx.saved_tensors, cot, wrt)
                for k, n in enumerate(wrt):
                    out[5 + WRT.index(n)] = r.grad[k]
            return tuple(out)

        @staticmethod
        def jvp(ctx, t_mp, t_tps, t_names, t_theta, t_rho, *tangents):
            if t_rho is not None:
                raise NotImplementedError("forward-mode tangent on rho: the air density is held fixed")
            parts = []
            if t_theta is not None:
                direction = {n: float(t) for n, t in zip(ctx.names, t_theta.tolist())}
                parts.append(param_tangents_out(param_jvp(ctx.mp, ctx.tps, ctx.saved_tensors, [direction])))
            state = {n: t.contiguous() for n, t in zip(WRT, tangents) if t is not None}
            if state or not parts:
                parts.append(tangents_out(jvp(ctx.mp, ctx.tps, ctx.saved_tensors, state)))
            return parts[0] if len(parts) == 1 else tuple(a + b for a, b in zip(*parts))
    F.__name__ = F.__qualname__ = name
    return F


_WarmRain2MTheta = _theta_function(
    "WarmRainTendencies2MTheta", _bt.JACOBIAN_WRT,
    lambda mp, tps, cols: _bt.bulk_microphysics_tendencies(_bt.Microphysics2Moment(), mp, tps, *cols)[:4],
    lambda mp, tps, cols, cotangents, wrt: _bt.warm_rain_vjp_2m(mp, tps, *cols, cotangents, wrt=wrt),
    lambda mp, tps, cols, tangents: _bt.warm_rain_jvp_2m(mp, tps, *cols, tangents),
    lambda mp, tps, cols, cotangents, names: _bt.warm_rain_param_vjp_2m(mp, tps, *cols, cotangents, names),
    lambda mp, tps, cols, directions: _bt.warm_rain_param_jvp_2m(mp, tps, *cols, directions))

_Tendencies1MTheta = _theta_function(
    "Tendencies1MTheta", _m1.JACOBIAN_WRT_1M,
    lambda mp, tps, cols: _m1.bulk_microphysics_tendencies_1m(_m1.Instantaneous(), _m1.Microphysics1Moment(), mp, tps, *cols),
    lambda mp, tps, cols, cotangents, wrt: _m1.vjp_1m(mp, tps, *cols, cotangents, wrt=wrt),
    lambda mp, tps, cols, tangents: _m1.jvp_1m(mp, tps, *cols, tangents),
    lambda mp, tps, cols, cotangents, names: _m1.param_vjp_1m(mp, tps, *cols, cotangents, names),
    lambda mp, tps, cols, directions: _m1.param_jvp_1m(mp, tps, *cols, directions))


# the column step as a function of theta: the parameter objects in the `mp` slot are a _ColumnStep whose structs were all rebuilt with theta
_Column2MTheta = _theta_function(
    "ColumnTendenciesSedimentation2MTheta", _bt.JACOBIAN_WRT, _column_primal,
    lambda step, tps, cols, cotangents, wrt: _bt.column_vjp_2m(step.mp, tps, step.inv_dz, *cols, cotangents[:4], cotangents[4], wrt=wrt, **step.options),
    lambda step, tps, cols, tangents: _bt.column_jvp_2m(step.mp, tps, step.inv_dz, *cols, tangents, **step.options),
    lambda step, tps, cols, cotangents, names: _bt.column_param_vjp_2m(step.mp, tps, step.inv_dz, *cols, cotangents[:4], cotangents[4], names, **step.options),
    lambda step, tps, cols, directions: _bt.column_param_jvp_2m(step.mp, tps, step.inv_dz, *cols, directions, **step.options),
    tangents_out=lambda r: (*(r.jvp[o] for o in range(4)), r.jvp_precip),
    param_tangents_out=lambda r: (*(r.jvp[0][o] for o in range(4)), r.jvp_precip[0]))


_Column1MTheta = _theta_function(
    "ColumnTendenciesSedimentation1MTheta", _m1.JACOBIAN_WRT_1M,
    lambda step, tps, cols: tuple(_m1.column_tendencies_sedimentation_1m(_m1.Instantaneous(), _m1.Microphysics1Moment(), step.mp[0], tps, *step.mp[1:],
                                                                          step.inv_dz, *cols)),
    lambda step, tps, cols, cotangents, wrt: _m1.column_vjp_1m(step.mp[0], tps, *step.mp[1:], step.inv_dz, *cols, cotangents[:4], cotangents[4], cotangents[5],
                                                                wrt=wrt),
    lambda step, tps, cols, tangents: _m1.column_jvp_1m(step.mp[0], tps, *step.mp[1:], step.inv_dz, *cols, tangents),
    lambda step, tps, cols, cotangents, names: _m1.column_param_vjp_1m(step.mp[0], tps, *step.mp[1:], step.inv_dz, *cols, cotangents[:4], cotangents[4],
                                                                        cotangents[5], names),
    lambda step, tps, cols, directions: _m1.column_param_jvp_1m(step.mp[0], tps, *step.mp[1:], step.inv_dz, *cols, directions),
    tangents_out=lambda r: (*(r.jvp[o] for o in range(4)), r.jvp_precip_rai, r.jvp_precip_sno),
    param_tangents_out=lambda r: (*(r.jvp[0][o] for o in range(4)), r.jvp_precip_rai[0], r.jvp_precip_sno[0]))


def _overridden(base, td, names, values):
    """The overrides `base` with names[k] = values[k]; "name[i]" sets entry i of a vector-valued name (the Chen-2022 tables of the 1-moment column step)."""
    ov = dict(base)
    for name, value in zip(names, values):
        key, idx = _P.split_indexed_name(name)
        if idx is None:
            ov[key] = value
        else:
            entries = list(ov.get(key, td[key]))
            entries[idx] = value
            ov[key] = entries
    return ov


def _with_theta(mp, tps, theta, names, known=None):
    """(parameter object, thermodynamics struct, names) rebuilt from mp's own dictionary with names[k] = theta[k]; `tps` itself unless a name feeds it."""
    if not (isinstance(theta, torch.Tensor) and theta.device.type == "cpu" and theta.dtype == torch.float64 and theta.dim() == 1):
        raise TypeError("theta: a 1-D CPU float64 tensor expected (the parameter structs are host data)")
    names = tuple(names) if names is not None else ()
    if len(names) != theta.numel() or len(set(names)) != len(names) or not names:
        raise ValueError("names: one distinct ClimaParams name per element of theta expected")
    one_moment = isinstance(mp, _P.Microphysics1MParams)
    p = mp if one_moment else _bt._warm_rain(mp)
    if known is None:
        known = _P.MICROPHYSICS_1M_DIRECTION_NAMES if one_moment else _P.WARM_RAIN_2M_DIRECTION_FIELDS
    for n in names:
        if n not in known:
            raise ValueError(f"names: '{n}' feeds no floating field of the scheme's or the thermodynamics parameters")
    rebuild = (lambda td: _P.Microphysics1MParams(td, **{k: getattr(p.processes, k) for k in p.processes._defaults})) if one_moment else (lambda td: _P.WarmRainParams2M(td, p.is_limited))
    base = {k: p.td[k] for k in p.td.overridden}
    feeds_tps = any(f[0][0] == "tps" for n in names for f in [_P.WARM_RAIN_2M_DIRECTION_FIELDS.get(n, (("", "", 0),))])
    # the rebuild starts from the dictionary, so a struct that no longer is what its dictionary builds would silently lose the caller's edits: refuse it
    td0 = _P.create_toml_dict(p.td.FT, base)
    if bytes(rebuild(td0).c) != bytes(p.c):
        raise ValueError("theta: the fields of mp were changed after construction; put the values into the dictionary mp is built from (create_toml_dict)")
    if feeds_tps and bytes(_P.ThermodynamicsParameters(td0)) != bytes(tps):
        raise ValueError("theta: a thermodynamics name rebuilds tps from mp's dictionary, and tps is not what that dictionary builds")
    td = _P.create_toml_dict(p.td.FT, _overridden(base, p.td, names, theta.detach().tolist()))
    return rebuild(td), (_P.ThermodynamicsParameters(td) if feeds_tps else tps), names


def _column_with_theta(mp, tps, theta, names, vel_params, cloud_vel):
    """_with_theta for the column step: the two fall-speed structs are rebuilt from the same dictionary as `mp`, and one that this dictionary does not
    build is refused like an edited `mp`."""
    wr, tps_t, names = _with_theta(mp, tps, theta, names, known=_P.COLUMN_2M_DIRECTION_FIELDS)
    p = _bt._warm_rain(mp)
    td0 = _P.create_toml_dict(p.td.FT, {k: p.td[k] for k in p.td.overridden})
    if vel_params is not None and bytes(_P.rain_vel_params(td0)) != bytes(vel_params):
        raise ValueError("theta: vel_params is not what mp's dictionary builds; put the values into the dictionary mp is built from (create_toml_dict)")
    if cloud_vel is not None and bytes(_P.StokesRegimeVelType(td0)) != bytes(cloud_vel):
        raise ValueError("theta: cloud_vel is not what mp's dictionary builds; put the values into the dictionary mp is built from (create_toml_dict)")
    return wr, tps_t, names, _P.rain_vel_params(wr.td), (_P.StokesRegimeVelType(wr.td) if cloud_vel is not None else None)


def _column_1m_with_theta(mp, tps, stokes, chen_rain, chen_ice, theta, names):
    """_with_theta for the 1-moment column step: the Stokes struct and the two Chen-2022 tables are rebuilt from the same dictionary as `mp`, and one that
    this dictionary does not build is refused like an edited `mp`."""
    for n in names or ():
        if _P.split_indexed_name(n)[0] in _P._CHEN_FIXED_NAMES:
            raise ValueError(f"names: '{n}' is held fixed: it reaches the rain fall speed through Γ(b − b_ρ ρ + 4), which carries no tangent on the device")
    mp_t, tps_t, names = _with_theta(mp, tps, theta, names, known=_P.COLUMN_1M_DIRECTION_NAMES)
    td0 = _P.create_toml_dict(mp.td.FT, {k: mp.td[k] for k in mp.td.overridden})
    for what, given, build in (("stokes", stokes, _P.StokesRegimeVelType), ("chen_rain", chen_rain, _P.Chen2022VelTypeRain), ("chen_ice", chen_ice, _P.Chen2022VelTypeIce)):
        if bytes(build(td0)) != bytes(given):
            raise ValueError(f"theta: {what} is not what mp's dictionary builds; put the values into the dictionary mp is built from (create_toml_dict)")
    return mp_t, tps_t, names, _P.StokesRegimeVelType(mp_t.td), _P.Chen2022VelTypeRain(mp_t.td), _P.Chen2022VelTypeIce(mp_t.td)


def warm_rain_tendencies_2m(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, theta=None, names=None):
    """(dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt) of `cmx.bulk_microphysics_tendencies(Microphysics2Moment(), mp, tps, …)`, bit for bit, differentiable by
    torch with respect to T, q_tot, q_lcl, n_lcl, q_rai, n_rai (reverse and forward mode; module docstring) and, with `theta` (1-D CPU float64) and `names`
    (ClimaParams names, `cmx.parameters.WARM_RAIN_2M_DIRECTION_FIELDS`), with respect to those parameters: the structs are rebuilt from `mp`'s dictionary with
    names[k] = theta[k] (a thermodynamics name rebuilds `tps` from the same dictionary).  Because of that rebuild, an `mp` whose fields were edited after
    construction — or, with a thermodynamics name, a `tps` that is not what `mp`'s dictionary builds — is a ValueError, not a silently dropped edit."""
    _check_rho(rho)
    if theta is None:
        if names is not None:
            raise ValueError("names without theta")
        return _WarmRain2M.apply(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    wr, tps_t, names = _with_theta(mp, tps, theta, names)
    return _WarmRain2MTheta.apply(wr, tps_t, names, theta, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)


def column_tendencies_sedimentation_2m(mp, tps, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, *, vel=_bt.SB2006VelType, vel_params=None, cloud_vel=None,
                                       theta=None, names=None):
    """(dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt, precip_flux) of `cmx.column_tendencies_sedimentation(mp, tps, inv_dz, …, want_precip_flux=True)`, bit for
    bit — the tendencies with the sedimentation flux divergence, shape (n_col, n_lev), and the surface precipitation flux, shape (n_col,) — differentiable by
    torch with respect to T, q_tot, q_lcl, n_lcl, q_rai, n_rai: backward is ONE Jᵀḡ launch (`cmx.column_vjp_2m`, the cotangent of the precipitation flux
    included: `precip_flux.sum().backward()` fills `.grad` of the state), forward mode ONE J v launch (`cmx.column_jvp_2m`).  ρ and `inv_dz` are held fixed:
    asking for their gradient, or a forward-mode tangent on them, raises NotImplementedError.

    With `theta` (1-D CPU float64) and `names` (ClimaParams names, `cmx.parameters.COLUMN_2M_DIRECTION_FIELDS` — the fall-speed parameters included) also with
    respect to those parameters: ALL the structs — `mp`, `tps` if a name feeds it, the rain fall-speed struct and `cloud_vel` if given — are rebuilt from
    `mp`'s dictionary with names[k] = theta[k]; backward fills `theta.grad` with ONE `cmx.column_param_vjp_2m` call (plus the Jᵀḡ launch if a state column
    needs a gradient), forward mode with a tangent on `theta` calls `cmx.column_param_jvp_2m`.  A `vel_params` or `cloud_vel` that the dictionary does not
    build is a ValueError.  The Chen-2022 table is held fixed (no name reaches it)."""
    _check_rho(rho)
    if inv_dz.requires_grad or torch.autograd.forward_ad.unpack_dual(inv_dz).tangent is not None:
        raise NotImplementedError("inv_dz is held fixed: the column step is not differentiated with respect to the layer thickness")
    if theta is not None:
        wr, tps_t, names, velp, cv = _column_with_theta(mp, tps, theta, names, vel_params, cloud_vel)
        return _Column2MTheta.apply(_ColumnStep(wr, inv_dz, dict(vel=vel, vel_params=velp, cloud_vel=cv)), tps_t, names, theta, rho, T, q_tot, q_lcl, n_lcl,
                                    q_rai, n_rai)
    if names is not None:
        raise ValueError("names without theta")
    return _Column2M.apply(_ColumnStep(mp, inv_dz, dict(vel=vel, vel_params=vel_params, cloud_vel=cloud_vel)), tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)


def column_tendencies_sedimentation_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, *, theta=None, names=None):
    """(dq_lcl_dt, dq_icl_dt, dq_rai_dt, dq_sno_dt, precip_rai, precip_sno) of `cmx.column_tendencies_sedimentation_1m(Instantaneous(),
    Microphysics1Moment(), mp, tps, stokes, chen_rain, chen_ice, inv_dz, …)`, bit for bit — the tendencies with the sedimentation flux divergence, shape
    (n_col, n_lev), and the surface fluxes of rain and snow, shape (n_col,) — differentiable by torch with respect to T, q_tot, q_lcl, q_icl, q_rai, q_sno:
    backward is ONE Jᵀḡ launch (`cmx.column_vjp_1m`, the cotangents of both precipitation fluxes included: `(precip_rai.sum() + precip_sno.sum()).backward()`
    fills `.grad` of the state), forward mode ONE J v launch (`cmx.column_jvp_1m`).  ρ and `inv_dz` are held fixed: asking for their gradient, or a
    forward-mode tangent on them, raises NotImplementedError.

    With `theta` (1-D CPU float64) and `names` (`cmx.parameters.COLUMN_1M_DIRECTION_NAMES` — the Stokes fall speed, the sedimentation number concentrations,
    the apparent densities and the entries "name[i]" of the Chen-2022 tables included) also with respect to those parameters: ALL five structs are rebuilt
    from `mp`'s dictionary with names[k] = theta[k]; backward fills `theta.grad` in the launches of ONE `cmx.column_param_vjp_1m` call (plus the Jᵀḡ launch
    if a state column needs a gradient), forward mode with a tangent on `theta` calls `cmx.column_param_jvp_1m`.  A `stokes`, `chen_rain` or `chen_ice`
    that the dictionary does not build is a ValueError; b and b_ρ of the Chen-2022 rain table are held fixed (ValueError).  Without `theta` the function is
    what it is without these two arguments."""
    _check_rho(rho)
    if inv_dz.requires_grad or torch.autograd.forward_ad.unpack_dual(inv_dz).tangent is not None:
        raise NotImplementedError("inv_dz is held fixed: the column step is not differentiated with respect to the layer thickness")
    if theta is not None:
        mp_t, tps_t, names, st, cr, ci = _column_1m_with_theta(mp, tps, stokes, chen_rain, chen_ice, theta, names)
        return _Column1MTheta.apply(_ColumnStep((mp_t, st, cr, ci), inv_dz, {}), tps_t, names, theta, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    if names is not None:
        raise ValueError("names without theta")
    return _Column1M.apply(_ColumnStep((mp, stokes, chen_rain, chen_ice), inv_dz, {}), tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)


def tendencies_1m(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, theta=None, names=None):
    """(dq_lcl_dt, dq_icl_dt, dq_rai_dt, dq_sno_dt) of `cmx.bulk_microphysics_tendencies_1m(Instantaneous(), Microphysics1Moment(), mp, tps, …)`, bit for bit,
    differentiable by torch with respect to T, q_tot, q_lcl, q_icl, q_rai, q_sno (reverse and forward mode; module docstring) and, with `theta` (1-D CPU float64)
    and `names` (`cmx.parameters.MICROPHYSICS_1M_DIRECTION_NAMES`), with respect to those parameters; the rules of `warm_rain_tendencies_2m`.  Instantaneous mode only."""
    _check_rho(rho)
    if theta is None:
        if names is not None:
            raise ValueError("names without theta")
        return _Tendencies1M.apply(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    mp_t, tps_t, names = _with_theta(mp, tps, theta, names)
    return _Tendencies1MTheta.apply(mp_t, tps_t, names, theta, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
