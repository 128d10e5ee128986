"""The launch path the Jacobian wrappers share (bulk_tendencies.warm_rain_jacobian_2m, microphysics1m.jacobian_1m): `wrt` validation, `out=` handling,
the contiguity checks, the pointer tables of the ABI (include/cmx.h §(14), §(15)) and the call."""
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
