"""The launch path the Jacobian wrappers share (bulk_tendencies.warm_rain_jacobian_2m, microphysics1m.jacobian_1m) and that of the products with the
Jacobian (warm_rain_jvp_2m / warm_rain_vjp_2m, jvp_1m / vjp_1m): `wrt` validation, `out=` handling, the contiguity checks, the pointer tables of the ABI
(include/cmx.h §(14) – §(17)) and the call."""
import ctypes as C

import torch

from . import _lib
from ._cols import _check_cols, _fam_of, _ptr


def _jacobian(entry, params, flags, tps, cols, names, wrt_all, nout, wrt, with_tendencies, out, stream):
    """(jac, tendencies, wrt) of `entry`_f32 / _f64.  params: the parameter object of the entry (`.c`, `.fam`); cols / names: the state columns, rho first;
    wrt_all: the entry's differentiable inputs in ABI order; nout: its outputs."""
    wrt = tuple(wrt)
    for name in wrt:
        if name not in wrt_all:
            raise ValueError(f"wrt: unknown input '{name}' (one of {wrt_all}; rho is not differentiated)")
    if len(set(wrt)) != len(wrt):
        raise ValueError("wrt: an input is listed twice")
    if not wrt and not with_tendencies:
        raise ValueError("nothing to compute: wrt is empty and with_tendencies is False")
    ref = _check_cols(cols, names)
    fam = _fam_of(ref)
    if fam is not params.fam or not isinstance(tps, fam.thermo):
        raise TypeError("parameter float type does not match the state columns")
    jac, tend = out if out is not None else (None, None)
    if jac is None:
        jac = torch.empty((nout, len(wrt), *ref.shape), dtype=ref.dtype, device=ref.device)
    elif jac.shape != (nout, len(wrt), *ref.shape):
        raise ValueError(f"out: jac must have shape ({nout}, len(wrt), *rho.shape) = {(nout, len(wrt), *ref.shape)}")
    if with_tendencies:
        if tend is None:
            tend = torch.empty((nout, *ref.shape), dtype=ref.dtype, device=ref.device)
        elif tend.shape != (nout, *ref.shape):
            raise ValueError(f"out: tendencies must have shape ({nout}, *rho.shape) = {(nout, *ref.shape)}")
    elif tend is not None:
        raise ValueError("out: a tendencies tensor was given but with_tendencies is False")
    if wrt:
        _check_cols([ref] + [jac[o, k] for o in range(nout) for k in range(len(wrt))], ["rho"] + ["jac"] * (nout * len(wrt)))
    if tend is not None:
        _check_cols([ref] + [tend[o] for o in range(nout)], ["rho"] + ["tendencies"] * nout)
    ptrs = [None] * (nout * len(wrt_all))
    for k, name in enumerate(wrt):
        for o in range(nout):
            ptrs[o * len(wrt_all) + wrt_all.index(name)] = jac[o, k].data_ptr()
    jac_p = (C.c_void_p * len(ptrs))(*ptrs)
    tend_p = (C.c_void_p * nout)(*[tend[o].data_ptr() for o in range(nout)]) if tend is not None else None
    _lib.call(entry, fam, ref.device, C.byref(params.c), C.byref(tps), flags, ref.numel(), *[_ptr(t) for t in cols], jac_p, tend_p, stream=stream)
    return jac, tend, wrt


def _check_wrt(wrt, wrt_all, what="wrt"):
    wrt = tuple(wrt)
    for name in wrt:
        if name == "rho":
            raise ValueError(f"{what}: rho is not differentiated")
        if name not in wrt_all:
            raise ValueError(f"{what}: unknown input '{name}' (one of {wrt_all}; rho is not differentiated)")
    if len(set(wrt)) != len(wrt):
        raise ValueError(f"{what}: an input is listed twice")
    return wrt


def _prep_product(params, tps, cols, names):
    ref = _check_cols(cols, names)
    fam = _fam_of(ref)
    if fam is not params.fam or not isinstance(tps, fam.thermo):
        raise TypeError("parameter float type does not match the state columns")
    return ref, fam


def _out_pair(out, ref, shape_a, name_a, nout, with_tendencies):
    """(first output, tendencies) from `out=`: allocated where None, shapes checked, every leading slice contiguous."""
    a, tend = out if out is not None else (None, None)
    if a is None:
        a = torch.empty((*shape_a, *ref.shape), dtype=ref.dtype, device=ref.device)
    elif a.shape != (*shape_a, *ref.shape):
        raise ValueError(f"out: {name_a} must have shape {(*shape_a, *ref.shape)}")
    if with_tendencies:
        if tend is None:
            tend = torch.empty((nout, *ref.shape), dtype=ref.dtype, device=ref.device)
        elif tend.shape != (nout, *ref.shape):
            raise ValueError(f"out: tendencies must have shape ({nout}, *rho.shape) = {(nout, *ref.shape)}")
    elif tend is not None:
        raise ValueError("out: a tendencies tensor was given but with_tendencies is False")
    if a.shape[0]:
        _check_cols([ref] + [a[k] for k in range(a.shape[0])], ["rho"] + [name_a] * a.shape[0])
    if tend is not None:
        _check_cols([ref] + [tend[o] for o in range(nout)], ["rho"] + ["tendencies"] * nout)
    return a, tend


def _table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def _jvp(entry, params, flags, tps, cols, names, wrt_all, nout, tangents, with_tendencies, out, stream):
    """(jvp, tendencies) of `entry`_f32 / _f64.  tangents: {name of a differentiable input: tensor}; a missing name is a zero tangent (a NULL column)."""
    if not isinstance(tangents, dict):
        raise TypeError("tangents must be a dict: name of a differentiable input -> tensor")
    _check_wrt(tangents.keys(), wrt_all, "tangents")
    ref, fam = _prep_product(params, tps, cols, names)
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
    ref, fam = _prep_product(params, tps, cols, names)
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
