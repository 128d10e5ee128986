"""Parameter ensembles (include/cmx.h §29): E parameter sets in one launch.

`pack_2m` / `pack_1m` fold a sequence of parameter objects into an `EnsembleTable` — one constants block per member, on the host — and
`table.to(device)` puts it on a GPU; the table is reusable across calls and time steps.  The wrappers below then evaluate every member in one
launch: member e of every result equals, bit for bit, the single-entry wrapper called with member e's parameters on member e's state.

    tab = cmx.ensemble.pack_2m(mps, tps, vel=cmx.SB2006VelType).to("cuda")
    out = cmx.ensemble.warm_rain_tendencies_2m(tab, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)           # columns of shape (E, n)
    out = cmx.ensemble.warm_rain_tendencies_2m(tab, rho, T, ..., shared_state=True)                       # columns of shape (n,): one state, E parameter sets

All members of a table run one kernel instantiation; members that differ in a choice the library makes from parameter values (integer SB2006
exponents, fitted or general Γ of a Chen-2022 rain table, default 1-moment exponents) make the pack raise CmxStatusError(CMX_ERR_UNSUPPORTED).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _abi, _lib
from ._cols import _check_cols, _fam_of, _ptr
from ._jacobian import _check_step, _check_step_normal
from .bulk_tendencies import ColumnTendencies2M, SB2006VelType, WarmRainTendencies2M, _vel_flag, _warm_rain
from .microphysics1m import ColumnStep1M, Tendencies1M
from .parameters import Microphysics1MParams, rain_vel_params

_NAMES_2M = ("rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai")
_NAMES_1M = ("rho", "T", "q_tot", "q_lcl", "q_icl", "q_rai", "q_sno")


class EnsembleTable:
    """The descriptor (`desc`, a host struct) and the constants table (`table`, a uint8 tensor of len(self) · stride bytes) of one packed ensemble."""

    def __init__(self, fam, desc, table):
        self.fam, self.desc, self.table = fam, desc, table

    def __len__(self):
        return int(self.desc.n_members)

    @property
    def device(self):
        return self.table.device

    def to(self, device) -> "EnsembleTable":
        """The same ensemble with its table on `device` (the descriptor stays on the host)."""
        return EnsembleTable(self.fam, self.desc, self.table.to(device))


def _array(items, ctype, n, what):
    """A contiguous C array of n structs from one struct (broadcast) or a sequence of n."""
    if isinstance(items, ctype):
        items = [items] * n
    items = list(items)
    if len(items) != n:
        raise ValueError(f"{what}: {len(items)} entries for {n} members")
    for x in items:
        if not isinstance(x, ctype):
            raise TypeError(f"{what}: expected {ctype.__name__} (the struct of the members' float type), got {type(x).__name__}")
    return (ctype * n)(*items)


def _pack(fn_name, fam, n, args, flags):
    fn = getattr(_lib.lib(), f"{fn_name}_{fam.sfx}")
    stride = getattr(_lib.lib(), f"{fn_name.replace('_pack', '_table_stride')}_{fam.sfx}")()
    table = torch.empty(n * stride, dtype=torch.uint8)
    desc = _abi.EnsembleDesc()
    _lib.check(fn.__name__, fn(*args, flags, n, C.c_void_p(table.data_ptr()), table.numel(), C.byref(desc)))
    return EnsembleTable(fam, desc, table)


def pack_2m(mps: Sequence, tps, *, vel=SB2006VelType, vel_params=None, cloud_vel=None, limited: Optional[bool] = None) -> EnsembleTable:
    """Packs the SB2006 members `mps` (Microphysics2MParams or WarmRainParams2M objects).  `tps`, `vel_params` (default:
    `parameters.rain_vel_params(FT)`) and `cloud_vel` are one struct for all members or a sequence of one per member.  `vel` = None packs no fall
    speed (pointwise tendencies without vt_rai_* only); `cloud_vel` adds cloud-droplet sedimentation to the column step; `limited` defaults to the
    members' own `is_limited`, which must agree."""
    wrs = [_warm_rain(m) for m in mps]
    if not wrs:
        raise ValueError("an ensemble needs at least one member")
    fam, n = wrs[0].fam, len(wrs)
    if any(w.fam is not fam for w in wrs):
        raise TypeError("all members must have one float type")
    if limited is None:
        limited = wrs[0].is_limited
        if any(w.is_limited != limited for w in wrs):
            raise ValueError("members disagree on is_limited")
    vflag = _vel_flag(vel)
    velp = None
    if vflag:
        velp = _array(vel_params if vel_params is not None else rain_vel_params(fam.sfx), fam.rain_vel, n, "vel_params")
    cv = _array(cloud_vel, fam.stokes_vel, n, "cloud_vel") if cloud_vel is not None else None
    args = ((fam.warm_rain_2m * n)(*[w.c for w in wrs]), _array(tps, fam.thermo, n, "tps"), velp, cv)
    return _pack("cmx_sb2006_ensemble_pack", fam, n, args, (_abi.CMX_SB2006_LIMITED if limited else 0) | vflag)


def pack_1m(mps: Sequence, tps, *, stokes=None, chen_rain=None, chen_ice=None) -> EnsembleTable:
    """Packs the 1-moment members `mps` (Microphysics1MParams objects with the same process options).  `tps` and the fall-speed parameters
    `stokes`, `chen_rain`, `chen_ice` (all three for the column step, none for a table of the pointwise tendencies only) are one struct for all
    members or a sequence of one per member."""
    mps = list(mps)
    if not mps:
        raise ValueError("an ensemble needs at least one member")
    if any(not isinstance(m, Microphysics1MParams) for m in mps):
        raise TypeError("mps must be Microphysics1MParams objects")
    fam, n = mps[0].fam, len(mps)
    if any(m.fam is not fam for m in mps):
        raise TypeError("all members must have one float type")
    if any(m.flags != mps[0].flags for m in mps):
        raise ValueError("members disagree on the process options")
    given = [x is not None for x in (stokes, chen_rain, chen_ice)]
    if any(given) and not all(given):
        raise TypeError("stokes, chen_rain and chen_ice: all three (the column step) or none (the pointwise tendencies only)")
    sed = (None, None, None)
    if all(given):
        sed = (_array(stokes, fam.stokes_vel, n, "stokes"), _array(chen_rain, fam.chen2022_rain_vel, n, "chen_rain"),
               _array(chen_ice, fam.chen2022_ice_vel, n, "chen_ice"))
    args = ((fam.microphysics_1m * n)(*[m.c for m in mps]), _array(tps, fam.thermo, n, "tps"), *sed)
    return _pack("cmx_mp1m_ensemble_pack", fam, n, args, mps[0].flags)


def _state(table, scheme, cols, names, shared_state, dims):
    """Validates the state columns of a call: shape (E, *dims) member-major or dims with `shared_state`.  Returns (ref, fam, per-member shape)."""
    if not isinstance(table, EnsembleTable) or table.desc.scheme != scheme:
        raise TypeError("table: an EnsembleTable packed for this scheme (pack_2m / pack_1m)")
    ref = _check_cols(cols, names)
    fam = _fam_of(ref)
    if fam is not table.fam:
        raise TypeError("the table's float type does not match the state columns")
    if table.table.device != ref.device:
        raise ValueError("the table must be on the device of the state columns (table.to(device))")
    want = dims if shared_state else dims + 1
    if ref.dim() != want:
        raise ValueError(f"state columns must have {want} dimensions ({'' if shared_state else 'members, '}{'columns, levels' if dims == 2 else 'points'})")
    if not shared_state and ref.shape[0] != len(table):
        raise ValueError(f"state columns hold {ref.shape[0]} members, the table {len(table)}")
    return ref, fam, tuple(ref.shape if shared_state else ref.shape[1:])


def _ens_args(table, shared_state):
    return (C.byref(table.desc), C.c_void_p(table.table.data_ptr()), len(table), _abi.CMX_ENSEMBLE_SHARED_STATE if shared_state else 0)


def _check_out(out, shape, ref, names):
    for o, nm in zip(out, names):
        if o is not None and (o.shape != shape or o.dtype != ref.dtype or o.device != ref.device or not o.is_contiguous()):
            raise ValueError(f"out.{nm}: expected a contiguous tensor of shape {tuple(shape)} with the state's dtype and device")


def warm_rain_tendencies_2m(table, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, *, shared_state=False, out: Optional[WarmRainTendencies2M] = None,
                            stream=None) -> WarmRainTendencies2M:
    """`bulk_microphysics_tendencies(Microphysics2Moment(), …)` for every member of `table`: columns of shape (E, n) in (or (n,) with
    `shared_state`), (E, n) out.  vt_rai_n / vt_rai_m are returned when the table was packed with a fall-speed scheme."""
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    ref, fam, (n,) = _state(table, _abi.CMX_ENSEMBLE_SCHEME_SB2006, cols, _NAMES_2M, shared_state, 1)
    shape = (len(table), n)
    want_vel = table.desc.vel_kind != 0
    if out is None:
        mk = lambda: torch.empty(shape, dtype=ref.dtype, device=ref.device)  # noqa: E731
        out = WarmRainTendencies2M(mk(), mk(), mk(), mk(), mk() if want_vel else None, mk() if want_vel else None)
    else:
        if any(o is None for o in out[:4]):
            raise ValueError("out: the four tendency columns are required")
        _check_out(out, shape, ref, WarmRainTendencies2M._fields)
    _lib.call("cmx_sb2006_warm_rain_tendencies_ensemble", fam, ref.device, *_ens_args(table, shared_state), n, *[_ptr(t) for t in cols],
              *[_ptr(o) for o in out], stream=stream)
    return out


def tendencies_1m(table, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, *, shared_state=False, out: Optional[Tendencies1M] = None,
                  stream=None) -> Tendencies1M:
    """`bulk_microphysics_tendencies_1m(Instantaneous(), …)` for every member of `table`: columns of shape (E, n) in (or (n,) with
    `shared_state`), (E, n) out."""
    cols = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    ref, fam, (n,) = _state(table, _abi.CMX_ENSEMBLE_SCHEME_MP1M, cols, _NAMES_1M, shared_state, 1)
    shape = (len(table), n)
    if out is None:
        out = Tendencies1M(*[torch.empty(shape, dtype=ref.dtype, device=ref.device) for _ in range(4)])
    else:
        if any(o is None for o in out):
            raise ValueError("out: the four tendency columns are required")
        _check_out(out, shape, ref, Tendencies1M._fields)
    _lib.call("cmx_mp1m_tendencies_ensemble", fam, ref.device, *_ens_args(table, shared_state), n, *[_ptr(t) for t in cols], *[_ptr(o) for o in out],
              stream=stream)
    return out


def _inv_dz(inv_dz, ref, n_lev):
    if inv_dz.dtype != ref.dtype or inv_dz.device != ref.device or inv_dz.numel() != n_lev or not inv_dz.is_contiguous():
        raise ValueError("inv_dz must be a contiguous device vector of n_lev values of the state dtype (shared by all members)")


def column_tendencies_sedimentation_2m(table, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, *, shared_state=False, want_precip_flux: bool = False,
                                       out: Optional[ColumnTendencies2M] = None, stream=None) -> ColumnTendencies2M:
    """`column_tendencies_sedimentation` for every member of `table`: state tensors of shape (E, n_col, n_lev) (or (n_col, n_lev) with
    `shared_state`), tendencies (E, n_col, n_lev), precip_flux (E, n_col).  The table must have been packed with a fall-speed scheme; cloud-droplet
    sedimentation runs when it was packed with `cloud_vel`."""
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    ref, fam, (n_col, n_lev) = _state(table, _abi.CMX_ENSEMBLE_SCHEME_SB2006, cols, _NAMES_2M, shared_state, 2)
    if table.desc.vel_kind == 0:
        raise ValueError("the column step needs a table packed with a rain fall-speed scheme (pack_2m(vel=SB2006VelType | Chen2022VelTypeRain))")
    _inv_dz(inv_dz, ref, n_lev)
    E = len(table)
    if out is None:
        out = ColumnTendencies2M(*[torch.empty((E, n_col, n_lev), dtype=ref.dtype, device=ref.device) for _ in range(4)],
                                 torch.empty((E, n_col), dtype=ref.dtype, device=ref.device) if want_precip_flux else None)
    else:
        if any(o is None for o in out[:4]):
            raise ValueError("out: the four tendency columns are required")
        _check_out(out[:4], (E, n_col, n_lev), ref, ColumnTendencies2M._fields)
        _check_out(out[4:], (E, n_col), ref, ("precip_flux",))
    _lib.call("cmx_sb2006_column_tendencies_sedimentation_ensemble", fam, ref.device, *_ens_args(table, shared_state), n_col, n_lev, _ptr(inv_dz),
              *[_ptr(t) for t in cols], *[_ptr(t) for t in out[:4]], _ptr(out.precip_flux), stream=stream)
    return out


def column_tendencies_sedimentation_1m(table, inv_dz, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, dt=None, nsub=0, *, q_min=None, shared_state=False,
                                       precip: bool = True, stream=None) -> ColumnStep1M:
    """`column_tendencies_sedimentation_1m` (the unshaped step) for every member of `table`: state tensors of shape (E, n_col, n_lev) (or
    (n_col, n_lev) with `shared_state`), tendencies (E, n_col, n_lev), precip_rai / precip_sno (E, n_col).  `nsub` = 0: Instantaneous tendencies;
    `nsub` ≥ 1 with `dt`: LinearizedAverage.  dt, nsub and q_min are shared by all members.  The table must have been packed with the fall-speed
    parameters."""
    cols = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    ref, fam, (n_col, n_lev) = _state(table, _abi.CMX_ENSEMBLE_SCHEME_MP1M, cols, _NAMES_1M, shared_state, 2)
    if not table.desc.sedimentation:
        raise ValueError("the column step needs a table packed with stokes, chen_rain and chen_ice")
    _inv_dz(inv_dz, ref, n_lev)
    lin = int(nsub) > 0
    if lin:
        if dt is None or not dt > 0:
            raise ValueError("nsub >= 1 (LinearizedAverage) needs dt > 0")
        if q_min is None:
            from .parameters import DEFAULT_PARAMETERS
            q_min = DEFAULT_PARAMETERS["specific_humidity_minimum"]
    elif dt is not None:
        raise TypeError("nsub = 0 (Instantaneous) takes no dt")
    E = len(table)
    out = [torch.empty((E, n_col, n_lev), dtype=ref.dtype, device=ref.device) for _ in range(4)]
    pr = [torch.empty((E, n_col), dtype=ref.dtype, device=ref.device) if precip else None for _ in range(2)]
    in_p = (C.c_void_p * 7)(*[c.data_ptr() for c in cols])
    out_p = (C.c_void_p * 4)(*[o.data_ptr() for o in out])
    _lib.call("cmx_mp1m_column_tendencies_sedimentation_ensemble", fam, ref.device, *_ens_args(table, shared_state), q_min if lin else 0.0,
              dt if lin else 0.0, int(nsub) if lin else 0, n_col, n_lev, _ptr(inv_dz), in_p, out_p, _ptr(pr[0]), _ptr(pr[1]), stream=stream)
    return ColumnStep1M(*out, *pr)


def _not_state(outs, cols):
    state = {c.data_ptr() for c in cols}
    if any(o is not None and o.data_ptr() in state for o in outs):
        raise ValueError("an output column must not be a state column: this step is not in place")


def column_implicit_step_2m(table, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dt, nsub=1, nonnegative=True, *, shared_state=False,
                            want_precip_flux: bool = False, out: Optional[ColumnTendencies2M] = None, stream=None) -> ColumnTendencies2M:
    """`column_implicit_step_2m` — the sub-stepped implicit average with backward-Euler sedimentation, stable and positive at any Courant number — for
    every member of `table` in one launch: state tensors of shape (E, n_col, n_lev) (or (n_col, n_lev) with `shared_state`), tendencies
    (E, n_col, n_lev), precip_flux (E, n_col).  `inv_dz`, `dt`, `nsub` and `nonnegative` are shared by all members; the latent heating of the substeps
    uses each member's own thermodynamics parameters.  The table must have been packed with a fall-speed scheme; cloud-droplet sedimentation runs when
    it was packed with `cloud_vel`.  An output must not be a state tensor."""
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    dt, nsub = _check_step(dt, nsub)
    ref, fam, (n_col, n_lev) = _state(table, _abi.CMX_ENSEMBLE_SCHEME_SB2006, cols, _NAMES_2M, shared_state, 2)
    if table.desc.vel_kind == 0:
        raise ValueError("the column step needs a table packed with a rain fall-speed scheme (pack_2m(vel=SB2006VelType | Chen2022VelTypeRain))")
    _check_step_normal(dt, nsub, ref.dtype)
    _inv_dz(inv_dz, ref, n_lev)
    E = len(table)
    if out is None:
        out = ColumnTendencies2M(*[torch.empty((E, n_col, n_lev), dtype=ref.dtype, device=ref.device) for _ in range(4)],
                                 torch.empty((E, n_col), dtype=ref.dtype, device=ref.device) if want_precip_flux else None)
    else:
        if any(o is None for o in out[:4]):
            raise ValueError("out: the four tendency columns are required")
        _check_out(out[:4], (E, n_col, n_lev), ref, ColumnTendencies2M._fields)
        _check_out(out[4:], (E, n_col), ref, ("precip_flux",))
        _not_state(out, cols)
    _lib.call("cmx_sb2006_column_implicit_step_ensemble", fam, ref.device, *_ens_args(table, shared_state), dt, nsub,
              _abi.CMX_STEP_NONNEGATIVE if nonnegative else 0, n_col, n_lev, _ptr(inv_dz), *[_ptr(t) for t in cols], *[_ptr(t) for t in out[:4]],
              _ptr(out.precip_flux), stream=stream)
    return out


def column_implicit_step_1m(table, inv_dz, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, dt, nsub=1, nonnegative=True, *, shared_state=False,
                            precip: bool = True, stream=None) -> ColumnStep1M:
    """`column_implicit_step_1m` for every member of `table` in one launch: state tensors of shape (E, n_col, n_lev) (or (n_col, n_lev) with
    `shared_state`), tendencies (E, n_col, n_lev), precip_rai / precip_sno (E, n_col).  `inv_dz`, `dt`, `nsub` and `nonnegative` are shared by all
    members; the latent heating of the substeps uses each member's own thermodynamics parameters.  The table must have been packed with the
    fall-speed parameters."""
    cols = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    dt, nsub = _check_step(dt, nsub)
    ref, fam, (n_col, n_lev) = _state(table, _abi.CMX_ENSEMBLE_SCHEME_MP1M, cols, _NAMES_1M, shared_state, 2)
    if not table.desc.sedimentation:
        raise ValueError("the column step needs a table packed with stokes, chen_rain and chen_ice")
    _check_step_normal(dt, nsub, ref.dtype)
    _inv_dz(inv_dz, ref, n_lev)
    E = len(table)
    out = [torch.empty((E, n_col, n_lev), dtype=ref.dtype, device=ref.device) for _ in range(4)]
    pr = [torch.empty((E, n_col), dtype=ref.dtype, device=ref.device) if precip else None for _ in range(2)]
    in_p = (C.c_void_p * 7)(*[c.data_ptr() for c in cols])
    out_p = (C.c_void_p * 4)(*[o.data_ptr() for o in out])
    _lib.call("cmx_mp1m_column_implicit_step_ensemble", fam, ref.device, *_ens_args(table, shared_state), dt, nsub,
              _abi.CMX_STEP_NONNEGATIVE if nonnegative else 0, n_col, n_lev, _ptr(inv_dz), in_p, out_p, _ptr(pr[0]), _ptr(pr[1]), stream=stream)
    return ColumnStep1M(*out, *pr)
