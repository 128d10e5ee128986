"""The launch path the Jacobian wrappers share (bulk_tendencies.warm_rain_jacobian_2m, microphysics1m.jacobian_1m) and that of the products with the
Jacobian (warm_rain_jvp_2m / warm_rain_vjp_2m, jvp_1m / vjp_1m) and of the linearly implicit tendencies (warm_rain_implicit_tendencies_2m,
implicit_tendencies_1m) and their sub-stepped average (warm_rain_implicit_average_2m, implicit_average_1m): `wrt` validation, `out=` handling, the contiguity checks, the pointer tables of the ABI (include/cmx.h §(14) – §(19)) and the call."""
import ctypes as C
import itertools
import math

import torch

from . import _abi, _lib
from ._cols import _check_cols, _fam_of, _ptr
from .parameters import parameter_direction


def _check_wrt(wrt, wrt_all, what="wrt", rho_is_unknown=False):
    wrt = tuple(wrt)
    for name in wrt:
        if name == "rho" and not rho_is_unknown:
            raise ValueError(f"{what}: rho is not differentiated")
        if name not in wrt_all:
            raise ValueError(f"{what}: unknown input '{name}' (one of {wrt_all}; rho is not differentiated)")
    if len(set(wrt)) != len(wrt):
        raise ValueError(f"{what}: an input is listed twice")
    return wrt


def _prep(params, tps, cols, names):
    ref = _check_cols(cols, names)
    fam = _fam_of(ref)
    if fam is not params.fam or not isinstance(tps, fam.thermo):
        raise TypeError("parameter float type does not match the state columns")
    return ref, fam


def _out_pair(out, ref, shape_a, name_a, nout, with_tendencies, shape_text=""):
    """(first output, tendencies) from `out=`: allocated where None, shapes checked, every slice a[i…] over the leading shape_a checked like a column."""
    a, tend = out if out is not None else (None, None)
    if a is None:
        a = torch.empty((*shape_a, *ref.shape), dtype=ref.dtype, device=ref.device)
    elif a.shape != (*shape_a, *ref.shape):
        raise ValueError(f"out: {name_a} must have shape {shape_text}{(*shape_a, *ref.shape)}")
    if with_tendencies:
        if tend is None:
            tend = torch.empty((nout, *ref.shape), dtype=ref.dtype, device=ref.device)
        elif tend.shape != (nout, *ref.shape):
            raise ValueError(f"out: tendencies must have shape ({nout}, *rho.shape) = {(nout, *ref.shape)}")
    elif tend is not None:
        raise ValueError("out: a tendencies tensor was given but with_tendencies is False")
    slices = [a[idx] for idx in itertools.product(*map(range, shape_a))]
    if slices:
        _check_cols([ref] + slices, ["rho"] + [name_a] * len(slices))
    if tend is not None:
        _check_cols([ref] + [tend[o] for o in range(nout)], ["rho"] + ["tendencies"] * nout)
    return a, tend


def _table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def _jacobian(entry, params, flags, tps, cols, names, wrt_all, nout, wrt, with_tendencies, out, stream):
    """(jac, tendencies, wrt) of `entry`_f32 / _f64.  params: the parameter object of the entry (`.c`, `.fam`); cols / names: the state columns, rho first;
    wrt_all: the entry's differentiable inputs in ABI order; nout: its outputs."""
    wrt = _check_wrt(wrt, wrt_all, rho_is_unknown=True)
    if not wrt and not with_tendencies:
        raise ValueError("nothing to compute: wrt is empty and with_tendencies is False")
    ref, fam = _prep(params, tps, cols, names)
    jac, tend = _out_pair(out, ref, (nout, len(wrt)), "jac", nout, with_tendencies, f"({nout}, len(wrt), *rho.shape) = ")
    columns = [None] * (nout * len(wrt_all))
    for k, name in enumerate(wrt):
        for o in range(nout):
            columns[o * len(wrt_all) + wrt_all.index(name)] = jac[o, k]
    _lib.call(entry, fam, ref.device, C.byref(params.c), C.byref(tps), flags, ref.numel(), *[_ptr(t) for t in cols], _table(columns),
              _table([tend[o] for o in range(nout)]) if tend is not None else None, stream=stream)
    return jac, tend, wrt


def _jvp(entry, params, flags, tps, cols, names, wrt_all, nout, tangents, with_tendencies, out, stream):
    """(jvp, tendencies) of `entry`_f32 / _f64.  tangents: {name of a differentiable input: tensor}; a missing name is a zero tangent (a NULL column)."""
    if not isinstance(tangents, dict):
        raise TypeError("tangents must be a dict: name of a differentiable input -> tensor")
    _check_wrt(tangents.keys(), wrt_all, "tangents")
    ref, fam = _prep(params, tps, cols, names)
    given = [(k, v) for k, v in tangents.items() if v is not None]
    if given:
        _check_cols([ref] + [v for _, v in given], ["rho"] + [f"tangent of {k}" for k, _ in given])
    jvp, tend = _out_pair(out, ref, (nout,), "jvp", nout, with_tendencies)
    tan_p = _table([tangents.get(name) for name in wrt_all])
    _lib.call(entry, fam, ref.device, C.byref(params.c), C.byref(tps), flags, ref.numel(), *[_ptr(t) for t in cols], tan_p,
              _table([jvp[o] for o in range(nout)]), _table([tend[o] for o in range(nout)]) if tend is not None else None, stream=stream)
    return jvp, tend


def _vjp(entry, params, flags, tps, cols, names, wrt_all, nout, cotangents, wrt, with_tendencies, out, stream):
    """(grad, tendencies, wrt) of `entry`_f32 / _f64.  cotangents: a sequence of `nout` tensors or None (None: that output is not part of the sum)."""
    wrt = _check_wrt(wrt, wrt_all)
    cotangents = list(cotangents)
    if len(cotangents) != nout:
        raise ValueError(f"cotangents: {nout} tensors (or None) expected, one per output")
    if not wrt and not with_tendencies:
        raise ValueError("nothing to compute: wrt is empty and with_tendencies is False")
    ref, fam = _prep(params, tps, cols, names)
    given = [(o, g) for o, g in enumerate(cotangents) if g is not None]
    if given:
        _check_cols([ref] + [g for _, g in given], ["rho"] + [f"cotangent {o}" for o, _ in given])
    grad, tend = _out_pair(out, ref, (len(wrt),), "grad", nout, with_tendencies)
    grads = [None] * len(wrt_all)
    for k, name in enumerate(wrt):
        grads[wrt_all.index(name)] = grad[k]
    _lib.call(entry, fam, ref.device, C.byref(params.c), C.byref(tps), flags, ref.numel(), *[_ptr(t) for t in cols], _table(cotangents), _table(grads),
              _table([tend[o] for o in range(nout)]) if tend is not None else None, stream=stream)
    return grad, tend, wrt


def _implicit(entry, params, flags, tps, cols, names, nout, dt, with_tendencies, out, stream):
    """(implicit, tendencies) of `entry`_f32 / _f64: r = (I − dt·J)⁻¹ f over the `nout` species of the scheme.  dt: a finite number ≥ 0."""
    dt = float(dt)
    if not (math.isfinite(dt) and dt >= 0.0):
        raise ValueError("dt must be finite and >= 0")
    ref, fam = _prep(params, tps, cols, names)
    impl, tend = _out_pair(out, ref, (nout,), "implicit", nout, with_tendencies)
    _lib.call(entry, fam, ref.device, C.byref(params.c), C.byref(tps), flags, ref.numel(), *[_ptr(t) for t in cols], dt,
              _table([impl[o] for o in range(nout)]), _table([tend[o] for o in range(nout)]) if tend is not None else None, stream=stream)
    return impl, tend


def _check_step(dt, nsub):
    """(dt, nsub) of an average entry as it takes them: dt finite and > 0, nsub 1 … CMX_IMPLICIT_AVERAGE_MAX_NSUB."""
    dt = float(dt)
    if not (math.isfinite(dt) and dt > 0.0):
        raise ValueError("dt must be finite and > 0")
    if isinstance(nsub, bool) or int(nsub) != nsub or not 1 <= int(nsub) <= _abi.CMX_IMPLICIT_AVERAGE_MAX_NSUB:
        raise ValueError(f"nsub must be an integer from 1 to {_abi.CMX_IMPLICIT_AVERAGE_MAX_NSUB}")
    return dt, int(nsub)


def _check_step_normal(dt, nsub, dtype):
    """dt / nsub and 1 / dt must be normal numbers of the state's float type."""
    # h = dt / nsub and 1 / dt as the entry forms them in the float type (a quotient of two Float32 values formed in double and rounded once more is the Float32 quotient)
    rnd, tiny, huge = ((lambda v: C.c_float(v).value), 2.0 ** -126, 2.0 ** 128 * (1 - 2.0 ** -24)) if dtype == torch.float32 else ((lambda v: v), 2.0 ** -1022, 1.7976931348623157e308)
    dt_f = rnd(dt)
    if not (tiny <= dt_f <= huge and tiny <= rnd(dt_f / nsub) <= huge and tiny <= rnd(1.0 / dt_f) <= huge):
        raise ValueError(f"dt / nsub and 1 / dt must be normal numbers of {dtype}")


def _implicit_average(entry, params, flags, tps, cols, names, nout, dt, nsub, nonnegative, out, stream):
    """average of `entry`_f32 / _f64: (s_end − s_start)/dt over `nsub` linearly implicit substeps of the `nout` species.  dt: finite and > 0 (and dt/nsub and
    1/dt normal numbers of the float type); nsub: 1 … CMX_IMPLICIT_AVERAGE_MAX_NSUB."""
    dt, nsub = _check_step(dt, nsub)
    ref, fam = _prep(params, tps, cols, names)
    _check_step_normal(dt, nsub, ref.dtype)
    avg, _ = _out_pair((out, None), ref, (nout,), "average", nout, False)
    _lib.call(entry, fam, ref.device, C.byref(params.c), C.byref(tps), flags, ref.numel(), *[_ptr(t) for t in cols], dt, nsub,
              _abi.CMX_STEP_NONNEGATIVE if nonnegative else 0, _table([avg[o] for o in range(nout)]), stream=stream)
    return avg


def _param_directions(params, directions):
    """The direction tables of the ABI (include/cmx.h §22, §23) from a sequence whose members are {ClimaParams name: weight} mappings or (d_params, d_thermo)
    pairs of `parameters.parameter_direction`.  params: the parameter object of the entry (`.c`, `.fam`)."""
    pairs = [parameter_direction(params, d) if isinstance(d, dict) else tuple(d) for d in directions]
    if not pairs:
        raise ValueError("directions: at least one direction expected")
    for a, b in pairs:
        if not isinstance(a, type(params.c)) or not isinstance(b, params.fam.thermo):
            raise TypeError("directions: (d_params, d_thermo) structs of the parameters' float type, or {name: weight} mappings")
    return (type(params.c) * len(pairs))(*[a for a, _ in pairs]), (params.fam.thermo * len(pairs))(*[b for _, b in pairs])


def _param_jvp(entry, params, flags, tps, cols, names, nout, directions, with_tendencies, out, stream):
    """(jvp, tendencies) of `entry`_f32 / _f64: jvp of shape (len(directions), nout, *rho.shape).  More than CMX_PARAM_MAX_DIRS directions are several calls
    of the entry (the tendencies are the first call's)."""
    ref, fam = _prep(params, tps, cols, names)
    d_p, d_tps = _param_directions(params, directions)
    ndir = len(d_p)
    jvp, tend = _out_pair(out, ref, (ndir, nout), "jvp", nout, with_tendencies, f"(len(directions), {nout}, *rho.shape) = ")
    for d0 in range(0, ndir, _abi.CMX_PARAM_MAX_DIRS):
        nd = min(_abi.CMX_PARAM_MAX_DIRS, ndir - d0)
        _lib.call(entry, fam, ref.device, C.byref(params.c), C.byref(tps), flags, ref.numel(), *[_ptr(t) for t in cols], nd, C.byref(d_p[d0]), C.byref(d_tps[d0]),
                  _table([jvp[d, o] for d in range(d0, d0 + nd) for o in range(nout)]),
                  _table([tend[o] for o in range(nout)]) if tend is not None and d0 == 0 else None, stream=stream)
    return jvp, tend


def _param_vjp(entry, params, flags, tps, cols, names, nout, cotangents, wrt, with_tendencies, out, stream):
    """(grad, tendencies, wrt) of `entry`_f32 / _f64: grad a float64 tensor of shape (len(wrt),) on the state's device.  wrt: ClimaParams names (one-hot
    directions) or directions as for _param_jvp.  The workspace is allocated here per call (the package keeps no cached device scratch) and reused by the
    calls of one invocation, which are ordered on the stream."""
    ref, fam = _prep(params, tps, cols, names)
    wrt = tuple(wrt)
    d_p, d_tps = _param_directions(params, [{w: 1.0} if isinstance(w, str) else w for w in wrt])
    cotangents = list(cotangents)
    if len(cotangents) != nout:
        raise ValueError(f"cotangents: {nout} tensors (or None) expected, one per output")
    given = [(o, g) for o, g in enumerate(cotangents) if g is not None]
    if given:
        _check_cols([ref] + [g for _, g in given], ["rho"] + [f"cotangent {o}" for o, _ in given])
    _, tend = _out_pair((None, out), ref, (0,), "grad", nout, with_tendencies)
    ndir = len(d_p)
    grad = torch.empty(ndir, dtype=torch.float64, device=ref.device)
    workspace = torch.empty(min(ndir, _abi.CMX_PARAM_MAX_DIRS) * _abi.CMX_PARAM_VJP_PARTIALS, dtype=torch.float64, device=ref.device)
    for d0 in range(0, ndir, _abi.CMX_PARAM_MAX_DIRS):
        nd = min(_abi.CMX_PARAM_MAX_DIRS, ndir - d0)
        _lib.call(entry, fam, ref.device, C.byref(params.c), C.byref(tps), flags, ref.numel(), *[_ptr(t) for t in cols], _table(cotangents), nd,
                  C.byref(d_p[d0]), C.byref(d_tps[d0]), _ptr(grad[d0:]), _ptr(workspace),
                  _table([tend[o] for o in range(nout)]) if tend is not None and d0 == 0 else None, stream=stream)
    return grad, tend, wrt
