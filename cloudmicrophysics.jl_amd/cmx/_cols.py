"""The wrappers' handling of state columns: float type, validation, pointers, and the shared driver of the `_fields` entries."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _abi, _lib


def _fam_of(t: torch.Tensor):
    if t.dtype == torch.float32:
        return _abi.F32
    if t.dtype == torch.float64:
        return _abi.F64
    raise TypeError(f"state columns must be float32 or float64, got {t.dtype}")


def _check_cols(cols, names):
    ref = cols[0]
    if not ref.is_cuda:
        raise ValueError("state columns must be resident on the GPU (torch device 'cuda'); cmx has no CPU path")
    for t, nm in zip(cols, names):
        if t.dtype != ref.dtype or t.device != ref.device or t.shape != ref.shape:
            raise ValueError(f"column {nm}: dtype/device/shape differ from {names[0]}")
        if not t.is_contiguous():
            raise ValueError(f"column {nm} must be contiguous (structure-of-arrays)")
    return ref


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _segments(t: torch.Tensor, name: str):
    """(n_seg, seg_len, stride) of a column given as a 1-D contiguous tensor or a 2-D (n_seg, seg_len) view whose rows are
    contiguous — e.g. `parent(field)[h, f, :]` of a ClimaCore VIJFH array seen from C order as (Nh, Nf, Nv·Ni·Nj)."""
    if t.dim() == 1 and t.stride(0) == 1:
        return 1, t.numel(), 0
    if t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1) and t.stride(0) >= t.shape[1]:
        return t.shape[0], t.shape[1], t.stride(0)
    raise TypeError(f"{name}: expected a contiguous 1-D column or a (n_seg, seg_len) view with contiguous rows")


def _fields_call(fn_name, params_c, tps, flags, cols, names, n_out, n_aos, out, aos, stream, extra=()):
    """Shared driver of the `_fields` entry points (segmented columns in; segmented columns or an (n, n_aos) array of rows out)."""
    ref = cols[0]
    fam = _fam_of(ref)
    n_seg, seg_len, _ = _segments(ref, names[0])
    strides = []
    for c, nm in zip(cols, names):
        if not c.is_cuda or c.device != ref.device or c.dtype != ref.dtype:
            raise TypeError(f"{nm}: all columns must live on the same GPU with the same dtype")
        ns, sl, st = _segments(c, nm)
        if (ns, sl) != (n_seg, seg_len):
            raise ValueError(f"{nm}: shape differs from {names[0]}")
        strides.append(st)
    n = n_seg * seg_len
    in_p = (C.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
    in_s = (C.c_int64 * len(cols))(*strides)
    out_p = out_s = aos_t = None
    if aos:
        if out is not None:
            raise TypeError("out is the SoA form; aos=True allocates the array-of-rows result")
        aos_t = torch.empty((n, n_aos), dtype=ref.dtype, device=ref.device)
    else:
        if out is None:
            out = [torch.empty(ref.shape, dtype=ref.dtype, device=ref.device) for _ in range(n_out)]
        ostr = []
        for o in out:
            ns, sl, st = _segments(o, "out")
            if (ns, sl) != (n_seg, seg_len) or o.dtype != ref.dtype or o.device != ref.device:
                raise ValueError("out: shape / dtype / device differs from the inputs")
            ostr.append(st)
        out_p = (C.c_void_p * n_out)(*[o.data_ptr() for o in out])
        out_s = (C.c_int64 * n_out)(*ostr)
    _lib.call(fn_name, fam, ref.device, C.byref(params_c), C.byref(tps), flags, *extra, n_seg, seg_len, in_p, in_s, out_p, out_s,
              C.c_void_p(aos_t.data_ptr()) if aos else None, stream=stream)
    return aos_t if aos else out
