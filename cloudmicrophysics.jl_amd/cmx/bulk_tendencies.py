"""Array entry points — host-side mirror of `CloudMicrophysics.BulkMicrophysicsTendencies` (BMT)
and of the per-process `CloudMicrophysics.Microphysics2M` (CM2) functions, evaluated over device
columns by the fused gfx950 kernels behind the C ABI (include/cmx.h).

Reference call being replaced (test/type_stability_tests.jl:131-137):

    BMT.bulk_microphysics_tendencies.(Ref(BMT.Microphysics2Moment()), Ref(mp), Ref(tps),
                                      ρ, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)

Here:

    bulk_microphysics_tendencies(Microphysics2Moment(), mp, tps, ρ, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)

with ρ… torch tensors resident in HBM; the result is a NamedTuple of columns (SoA) instead of the
reference's array of NamedTuples, with the same field names.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple
from typing import Optional

import torch

from . import _abi, _lib
from ._cols import _check_cols, _fam_of, _fields_call, _ptr, _segments
from ._jacobian import _check_step, _check_step_normal, _check_wrt, _implicit, _implicit_average, _jacobian, _jvp, _param_jvp, _param_vjp, _table, _vjp
from .parameters import Microphysics2MParams, WarmRainParams2M, column_parameter_direction, rain_vel_params


class Microphysics2Moment:
    """BMT.Microphysics2Moment — scheme tag (src/BulkMicrophysicsTendencies.jl:59-63)."""


class SB2006VelType:
    """velocity-scheme tag: CM2.rain_terminal_velocity(sb, ::SB2006VelType, …)  CM2:685-702"""
    flag = _abi.CMX_VEL_SB2006


class Chen2022VelTypeRain:
    """velocity-scheme tag: CM2.rain_terminal_velocity(sb, ::Chen2022VelTypeRain, …)  CM2:703-719"""
    flag = _abi.CMX_VEL_CHEN2022


WarmRainTendencies2M = namedtuple(
    "WarmRainTendencies2M",
    ["dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt", "vt_rai_n", "vt_rai_m"])

SB2006ProcessRates = namedtuple("SB2006ProcessRates", _abi.SB2006_PROCESS_COLUMNS)

# return of the 2M + P3 method (BMT:1079-1082)
Tendencies2MP3 = namedtuple(
    "Tendencies2MP3",
    ["dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt", "dq_ice_dt", "dn_ice_dt", "dq_rim_dt", "db_rim_dt", "dn_lcl_activation_dt"])


def _warm_rain(mp):
    if isinstance(mp, Microphysics2MParams):
        return mp.warm_rain
    if isinstance(mp, WarmRainParams2M):
        return mp
    raise TypeError("mp must be Microphysics2MParams or WarmRainParams2M")


def _vel_flag(vel):
    if vel is None:
        return 0
    flag = getattr(vel, "flag", None)
    if flag is None:
        raise TypeError("vel must be SB2006VelType, Chen2022VelTypeRain (class or instance) or None")
    return flag


def _bulk_tendencies_2m_p3(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, log_lambda, inpc_log_shift,
                           aspect_ratio, stream):
    """bulk_microphysics_tendencies(::Microphysics2Moment, mp{WR, P3IceParams}, …) — BMT:898-1083 behind
    cmx_microphysics_2m_p3_tendencies_*."""
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, log_lambda)
    ref = _check_cols(cols, ("rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai", "q_ice", "n_ice", "q_rim", "b_rim", "log_lambda"))
    fam = _fam_of(ref)
    if fam is not mp.fam or fam is not mp.ice.fam or not isinstance(tps, fam.thermo):
        raise TypeError("parameter float type does not match the state columns")
    if mp.ice.is_limited != mp.warm_rain.is_limited:
        raise ValueError("warm_rain and ice must use the same rain PSD variant (is_limited)")
    if inpc_log_shift is not None:
        _check_cols([ref, inpc_log_shift], ["rho", "inpc_log_shift"])
    outs = [torch.empty_like(ref) for _ in range(8)]
    out_p = (C.c_void_p * 8)(*[t.data_ptr() for t in outs])
    flags = mp.ice.flags | (0 if aspect_ratio else _abi.CMX_P3_NO_ASPECT_RATIO)
    _lib.call("cmx_microphysics_2m_p3_tendencies", fam, ref.device, C.byref(mp.warm_rain.c), C.byref(mp.ice.c), C.byref(tps), flags, ref.numel(),
              *[_ptr(t) for t in cols], _ptr(inpc_log_shift), out_p, stream=stream)
    return Tendencies2MP3(*outs, torch.zeros((), dtype=ref.dtype, device=ref.device).expand_as(ref))


def bulk_microphysics_tendencies(scheme, mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice=None, n_ice=None, q_rim=None,
                                 b_rim=None, log_lambda=None, inpc_log_shift=None, *, vel=None, vel_params=None, aspect_ratio=True,
                                 out: Optional[WarmRainTendencies2M] = None, stream=None):
    """2-moment tendencies over columns.

    With `mp = Microphysics2MParams(FT; with_ice = true)` and the P3 ice columns (q_ice, n_ice, q_rim, b_rim, logλ[, inpc_log_shift])
    this is the warm rain + P3 ice method, BMT:898-1083 (returns `Tendencies2MP3`).  Otherwise:

    2-moment warm-rain tendencies over columns — BMT:820-854 → warm_rain_tendencies_2m BMT:707-782.

    `vel` (None | SB2006VelType | Chen2022VelTypeRain) additionally fuses
    CM2.rain_terminal_velocity (CM2:685-719) into the same pass (two more output columns); `vel_params` = a `cmx_rain_vel` struct
    with non-default tables (default: `parameters.rain_vel_params(FT)`).
    `out` lets the caller provide the output columns (KA-kernel style, test/gpu_tests.jl:407-415).
    Asynchronous on `stream` (default: torch's current stream)."""
    if not isinstance(scheme, Microphysics2Moment):
        raise TypeError("only Microphysics2Moment() is on this path")
    if isinstance(mp, Microphysics2MParams) and mp.ice is not None:
        if any(x is None for x in (q_ice, n_ice, q_rim, b_rim, log_lambda)):
            raise TypeError("the 2M + P3 method needs q_ice, n_ice, q_rim, b_rim and log_lambda columns")
        if vel is not None or out is not None:
            raise TypeError("vel / out are options of the warm-rain method")
        return _bulk_tendencies_2m_p3(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, log_lambda,
                                      inpc_log_shift, aspect_ratio, stream)
    if q_ice is not None:
        raise TypeError("ice columns given but mp has no ice parameters (Microphysics2MParams(FT, with_ice=True))")
    wr = _warm_rain(mp)
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    ref = _check_cols(cols, ("rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai"))
    fam = _fam_of(ref)
    if fam is not wr.fam or not isinstance(tps, fam.thermo):
        raise TypeError("parameter float type does not match the state columns")
    vflag = _vel_flag(vel)
    if out is None:
        mk = lambda: torch.empty_like(ref)  # noqa: E731
        out = WarmRainTendencies2M(mk(), mk(), mk(), mk(), mk() if vflag else None, mk() if vflag else None)
    else:
        _check_cols([ref] + [o for o in out if o is not None], ["rho"] + ["out"] * 6)
    flags = (_abi.CMX_SB2006_LIMITED if wr.is_limited else 0) | vflag
    velp = (vel_params if vel_params is not None else rain_vel_params(fam.sfx)) if vflag else None
    if velp is not None and not isinstance(velp, fam.rain_vel):
        raise TypeError("vel_params must be the cmx_rain_vel struct of the state's float type")
    _lib.call("cmx_sb2006_warm_rain_tendencies", fam, ref.device, C.byref(wr.c), C.byref(tps), C.byref(velp) if velp is not None else None, flags,
              ref.numel(), *[_ptr(t) for t in cols], *[_ptr(o) for o in out], stream=stream)
    return out


WarmRainJacobian2M = namedtuple("WarmRainJacobian2M", ["jac", "tendencies", "wrt"])

JACOBIAN_OUTPUTS = _abi.SB2006_JAC_OUT
JACOBIAN_WRT = _abi.SB2006_JAC_WRT


def warm_rain_jacobian_2m(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, wrt=JACOBIAN_WRT, with_tendencies=False, *, out=None,
                          stream=None) -> WarmRainJacobian2M:
    """The Jacobian of the 2-moment warm-rain tendencies (BMT:820-854) with respect to the prognostic state — what the reference obtains with
    `ForwardDiff.jacobian` through `BMT.bulk_microphysics_tendencies(Microphysics2Moment(), mp, …)` (test/ad_compat_tests.jl:106-175) — behind
    `cmx_sb2006_warm_rain_jacobian_*`: the same point function as `bulk_microphysics_tendencies`, evaluated on forward-mode dual numbers in one kernel.

    `wrt`: the inputs to differentiate, any subset of `JACOBIAN_WRT` = ("T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai") in any order (ρ is held
    fixed).  Returns `WarmRainJacobian2M(jac, tendencies, wrt)`: `jac` is one contiguous tensor of shape (4, len(wrt), *rho.shape) with
    `jac[o, k]` = ∂`JACOBIAN_OUTPUTS[o]`/∂`wrt[k]` (its slices are the columns handed to the ABI; a column does not depend on which others are
    requested); `tendencies` is a (4, *rho.shape) tensor, bit-identical to `bulk_microphysics_tendencies` on the same columns, with
    `with_tendencies=True`, else None.  `out=(jac, tendencies)` lets the caller provide either tensor (None: allocated here; each slice
    `[o, k]` / `[o]` must be contiguous).  An implicit step solves (I − Δt·J) δ = Δt·f per point from these columns.
    Asynchronous on `stream` (default: torch's current stream)."""
    wr = _warm_rain(mp)
    return WarmRainJacobian2M(*_jacobian("cmx_sb2006_warm_rain_jacobian", wr, _abi.CMX_SB2006_LIMITED if wr.is_limited else 0, tps,
                                         (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai), ("rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai"), JACOBIAN_WRT,
                                         _abi.CMX_SB2006_JAC_NOUT, wrt, with_tendencies, out, stream))


WarmRainJvp2M = namedtuple("WarmRainJvp2M", ["jvp", "tendencies"])
WarmRainVjp2M = namedtuple("WarmRainVjp2M", ["grad", "tendencies", "wrt"])
_NAMES_2M = ("rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai")


def warm_rain_jvp_2m(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, tangents, with_tendencies=False, *, out=None, stream=None) -> WarmRainJvp2M:
    """J v of the 2-moment warm-rain tendencies behind `cmx_sb2006_warm_rain_jvp_*`: the directional derivative of the four tendencies along `tangents`,
    one evaluation of the point function on dual numbers seeded with the tangent — what a Jacobian-free Newton–Krylov matvec needs — without the 24
    columns of `warm_rain_jacobian_2m`.

    `tangents`: dict name -> tensor over `JACOBIAN_WRT`; a missing name is a zero tangent (ρ is held fixed: a `rho` tangent is a ValueError).  Returns
    `WarmRainJvp2M(jvp, tendencies)`: `jvp` of shape (4, *rho.shape) in the order of `JACOBIAN_OUTPUTS`; `tendencies` (4, *rho.shape), bit-identical to
    `bulk_microphysics_tendencies`, with `with_tendencies=True`, else None.  `out=(jvp, tendencies)` lets the caller provide either tensor.
    Asynchronous on `stream` (default: torch's current stream)."""
    wr = _warm_rain(mp)
    return WarmRainJvp2M(*_jvp("cmx_sb2006_warm_rain_jvp", wr, _abi.CMX_SB2006_LIMITED if wr.is_limited else 0, tps,
                               (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai), _NAMES_2M, JACOBIAN_WRT, _abi.CMX_SB2006_JAC_NOUT, tangents, with_tendencies, out,
                               stream))


def warm_rain_vjp_2m(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, cotangents, wrt=JACOBIAN_WRT, with_tendencies=False, *, out=None,
                     stream=None) -> WarmRainVjp2M:
    """Jᵀḡ of the 2-moment warm-rain tendencies behind `cmx_sb2006_warm_rain_vjp_*`: the gradient of Σ_o ḡ_o·out_o with respect to the inputs `wrt`, the
    Jacobian's columns contracted with the cotangents in registers — what `loss.backward()` needs (cmx.autograd) — without the 24 columns.

    `cotangents`: a sequence of 4 tensors or None in the order of `JACOBIAN_OUTPUTS`; None removes that output from the sum (a tensor of zeros does not:
    0·Inf is NaN, as contracting the Jacobian would give).  `wrt`: any subset of `JACOBIAN_WRT` in any order.  Returns `WarmRainVjp2M(grad, tendencies,
    wrt)`: `grad` of shape (len(wrt), *rho.shape); a gradient does not depend on which others are requested.  `tendencies`, `out=(grad, tendencies)` and
    `stream` as for `warm_rain_jvp_2m`."""
    wr = _warm_rain(mp)
    return WarmRainVjp2M(*_vjp("cmx_sb2006_warm_rain_vjp", wr, _abi.CMX_SB2006_LIMITED if wr.is_limited else 0, tps,
                               (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai), _NAMES_2M, JACOBIAN_WRT, _abi.CMX_SB2006_JAC_NOUT, cotangents, wrt,
                               with_tendencies, out, stream))


WarmRainParamJvp2M = namedtuple("WarmRainParamJvp2M", ["jvp", "tendencies"])
WarmRainParamVjp2M = namedtuple("WarmRainParamVjp2M", ["grad", "tendencies", "wrt"])


def warm_rain_param_jvp_2m(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, directions, with_tendencies=False, *, out=None, stream=None) -> WarmRainParamJvp2M:
    """The derivative of the 2-moment warm-rain tendencies with respect to the scheme's PARAMETERS along `directions`, behind
    `cmx_sb2006_warm_rain_param_jvp_*`: jvp[d, o] = Σ_p ∂`JACOBIAN_OUTPUTS[o]`/∂θ_p·δθ_p⁽ᵈ⁾ per point, the same point function as
    `bulk_microphysics_tendencies` on forward-mode duals whose tangents are those of the host-folded constants (exact forward mode, no difference quotient).

    `directions`: a sequence of {ClimaParams name: weight} mappings or of (d_warm_rain, d_thermo) pairs from `parameters.parameter_direction`; a one-hot
    mapping {name: 1.0} gives ∂out/∂name.  Returns `WarmRainParamJvp2M(jvp, tendencies)`: `jvp` of shape (len(directions), 4, *rho.shape); a column does not
    depend on which other directions are requested.  `tendencies` (4, *rho.shape) with `with_tendencies=True`, else None: bit-identical to
    `bulk_microphysics_tendencies` unless a direction moves one of the three exponents acnv.b, accr.c, self.d (then the general-exponent instantiation runs:
    agreement to the parity bound).  `out=(jvp, tendencies)` lets the caller provide either tensor.  More than `CMX_PARAM_MAX_DIRS` = 16 directions are
    several calls of the entry.  Asynchronous on `stream` (default: torch's current stream)."""
    wr = _warm_rain(mp)
    return WarmRainParamJvp2M(*_param_jvp("cmx_sb2006_warm_rain_param_jvp", wr, _abi.CMX_SB2006_LIMITED if wr.is_limited else 0, tps,
                                          (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai), _NAMES_2M, _abi.CMX_SB2006_JAC_NOUT, directions, with_tendencies, out, stream))


def warm_rain_param_vjp_2m(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, cotangents, wrt, with_tendencies=False, *, out=None,
                           stream=None) -> WarmRainParamVjp2M:
    """The gradient of L = Σ_points Σ_o ḡ_o·out_o with respect to the scheme's PARAMETERS, behind `cmx_sb2006_warm_rain_param_vjp_*` — what a calibration
    needs: grad[k] = dL/d`wrt[k]`, a deterministic reduction over the points in float64 (no atomics: bit-identical from run to run).

    `cotangents`: a sequence of 4 tensors or None in the order of `JACOBIAN_OUTPUTS`; None removes that output from the sum.  `wrt`: ClimaParams names
    (`parameters.WARM_RAIN_2M_DIRECTION_FIELDS`), or general directions as for `warm_rain_param_jvp_2m` (then grad[k] is the derivative along direction k).
    Returns `WarmRainParamVjp2M(grad, tendencies, wrt)`: `grad` a float64 tensor of shape (len(wrt),) on the state's device; a NaN in the state or a cotangent
    of any point makes it NaN.  `tendencies` as for `warm_rain_param_jvp_2m`; `out=tendencies` provides it.  The reduction's workspace (min(len(wrt), 16) × 1024
    float64) is allocated here per call: the package keeps no cached device scratch (cmx/_cols.py has none), and under graph capture the allocation comes from
    the capture's pool.  Asynchronous on `stream` (default: torch's current stream)."""
    wr = _warm_rain(mp)
    return WarmRainParamVjp2M(*_param_vjp("cmx_sb2006_warm_rain_param_vjp", wr, _abi.CMX_SB2006_LIMITED if wr.is_limited else 0, tps,
                                          (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai), _NAMES_2M, _abi.CMX_SB2006_JAC_NOUT, cotangents, wrt, with_tendencies, out,
                                          stream))


WarmRainImplicit2M = namedtuple("WarmRainImplicit2M", ["implicit", "tendencies"])


def warm_rain_implicit_tendencies_2m(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dt, with_tendencies=False, *, out=None,
                                     stream=None) -> WarmRainImplicit2M:
    """The tendency of a linearly implicit (Rosenbrock–Euler) step of the 2-moment warm-rain tendencies behind `cmx_sb2006_warm_rain_implicit_tendencies_*`:
    r = (I − dt·J)⁻¹ f per point, with f the four tendencies and J their Jacobian with respect to the species (q_lcl, n_lcl, q_rai, n_rai) at fixed ρ, T,
    q_tot — the 4 × 4 block of `warm_rain_jacobian_2m`, equilibrated and solved in registers in the pass that computes it (partial pivoting), instead of 20
    columns written, read back and handed to `torch.linalg.solve`.  The step is s ← s + dt·r; r = f in every bit at dt = 0.

    `dt`: seconds, finite and ≥ 0.  Returns `WarmRainImplicit2M(implicit, tendencies)`: `implicit` of shape (4, *rho.shape) in the order of
    `JACOBIAN_OUTPUTS`; `tendencies` (4, *rho.shape), bit-identical to `bulk_microphysics_tendencies`, with `with_tendencies=True`, else None.
    `out=(implicit, tendencies)` lets the caller provide either tensor; `implicit` may be a view of the four species columns themselves (in place).  A singular I − dt·J gives a non-finite r at that point only.  No sub-stepping, no
    positivity limiting of s + dt·r, no autograd through the solve.  Asynchronous on `stream` (default: torch's current stream)."""
    wr = _warm_rain(mp)
    return WarmRainImplicit2M(*_implicit("cmx_sb2006_warm_rain_implicit_tendencies", wr, _abi.CMX_SB2006_LIMITED if wr.is_limited else 0, tps,
                                         (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai), _NAMES_2M, _abi.CMX_SB2006_JAC_NOUT, dt, with_tendencies, out, stream))


def warm_rain_implicit_average_2m(mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dt, nsub=1, nonnegative=True, *, out=None, stream=None):
    """The average tendency of (q_lcl, n_lcl, q_rai, n_rai) over a time step `dt`, taken in `nsub` linearly implicit substeps inside one kernel
    (`cmx_sb2006_warm_rain_implicit_average_*`): each substep is s ← s + h·r with h = dt/nsub and r = `warm_rain_implicit_tendencies_2m(…, h).implicit` at the
    current state, T follows the latent heating of the substep (T += L_v/c_p·(Δq_lcl + Δq_rai)), ρ and q_tot stay fixed; the result is (s_end − s_start)/dt.
    `nonnegative=True` clips every substep: a species never ends one below 0, and one that was negative already never below where it started — without it the
    plain step leaves a species negative at a large share of states.  include/cmx.h §(19) has the definition, which is normative bit for bit.

    `dt`: seconds, finite and > 0; `nsub`: 1 … 64.  Returns a tensor of shape (4, *rho.shape) in the order of `JACOBIAN_OUTPUTS`; `out=` provides it and may be
    a view of the four species columns themselves (in place).  No autograd through the average.  Asynchronous on `stream` (default: torch's current stream)."""
    wr = _warm_rain(mp)
    return _implicit_average("cmx_sb2006_warm_rain_implicit_average", wr, _abi.CMX_SB2006_LIMITED if wr.is_limited else 0, tps,
                             (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai), _NAMES_2M, _abi.CMX_SB2006_JAC_NOUT, dt, nsub, nonnegative, out, stream)


AOS_FIELDS = ("dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt", "dq_ice_dt", "dq_rim_dt", "db_rim_dt", "dn_lcl_activation_dt")


def bulk_microphysics_tendencies_2m_p3_fields(scheme, mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, log_lambda,
                                              inpc_log_shift=None, *, aspect_ratio=True, out=None, stream=None):
    """The 2M + P3 method of `bulk_microphysics_tendencies` (BMT:898-1083) on the host model's own storage — the layout adapter of
    `cmx_microphysics_2m_p3_tendencies_fields_*`: every column is a contiguous 1-D tensor or a 2-D strided view (n_seg, seg_len) with
    contiguous rows (a component of a ClimaCore `VIJFH` field in place; each column may have its own row stride, all share the shape); the
    eight tendencies go into `out` (8 tensors of that shape, e.g. components of the tendency field; allocated contiguous if None).
    Bit-identical to the SoA call on the same states.  Returns `Tendencies2MP3`."""
    if not isinstance(scheme, Microphysics2Moment):
        raise TypeError("only Microphysics2Moment() is on this path")
    if not (isinstance(mp, Microphysics2MParams) and mp.ice is not None):
        raise TypeError("mp must be Microphysics2MParams(FT, with_ice=True)")
    names = ["rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai", "q_ice", "n_ice", "q_rim", "b_rim", "log_lambda"]
    cols = [rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, log_lambda]
    if inpc_log_shift is not None:
        names.append("inpc_log_shift"); cols.append(inpc_log_shift)
    ref = cols[0]
    fam = _fam_of(ref)
    if fam is not mp.fam or fam is not mp.ice.fam or not isinstance(tps, fam.thermo):
        raise TypeError("parameter float type does not match the state columns")
    if mp.ice.is_limited != mp.warm_rain.is_limited:
        raise ValueError("warm_rain and ice must use the same rain PSD variant (is_limited)")
    n_seg, seg_len, _ = _segments(ref, names[0])
    strides = []
    for c, nm in zip(cols, names):
        if not c.is_cuda or c.device != ref.device or c.dtype != ref.dtype:
            raise TypeError(f"{nm}: all columns must live on the same GPU with the same dtype")
        ns, sl, st = _segments(c, nm)
        if (ns, sl) != (n_seg, seg_len):
            raise ValueError(f"{nm}: shape differs from rho")
        strides.append(st)
    ptrs = [c.data_ptr() for c in cols]
    if inpc_log_shift is None:
        ptrs.append(None); strides.append(seg_len)
    if out is None:
        out = [torch.empty(ref.shape, dtype=ref.dtype, device=ref.device) for _ in range(8)]
    if len(out) != 8:
        raise ValueError("out: eight tendency columns")
    ostr = []
    for o in out:
        ns, sl, st = _segments(o, "out")
        if (ns, sl) != (n_seg, seg_len) or o.dtype != ref.dtype or o.device != ref.device:
            raise ValueError("out: shape / dtype / device differs from the inputs")
        ostr.append(st)
    in_p, in_s = (C.c_void_p * 13)(*ptrs), (C.c_int64 * 13)(*strides)
    out_p, out_s = (C.c_void_p * 8)(*[o.data_ptr() for o in out]), (C.c_int64 * 8)(*ostr)
    flags = mp.ice.flags | (0 if aspect_ratio else _abi.CMX_P3_NO_ASPECT_RATIO)
    _lib.call("cmx_microphysics_2m_p3_tendencies_fields", fam, ref.device, C.byref(mp.warm_rain.c), C.byref(mp.ice.c), C.byref(tps), flags, n_seg,
              seg_len, in_p, in_s, out_p, out_s, stream=stream)
    return Tendencies2MP3(*out, torch.zeros((), dtype=ref.dtype, device=ref.device).expand(ref.shape))


def bulk_microphysics_tendencies_fields(scheme, mp, tps, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, *, out=None, aos=False, stream=None):
    """The 2-moment warm-rain tendencies (BMT:820-854) on the host model's own storage — zero-copy layout adapters of
    `cmx_sb2006_warm_rain_tendencies_fields_*`:

    * inputs: each column is a contiguous 1-D tensor or a 2-D strided view (n_seg, seg_len) with contiguous rows — a component of a
      ClimaCore `VIJFH` field in place (every column may have its own row stride, all share the shape);
    * `aos=False`: the four tendencies go into `out` (4 tensors of the same shape, e.g. components of the tendency field; allocated
      contiguous if None) → `WarmRainTendencies2M` without velocities;
    * `aos=True`: returns the reference's result layout, an (n, 8) tensor whose rows are the NamedTuple
      (dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt, dq_ice_dt, dq_rim_dt, db_rim_dt, dn_lcl_activation_dt) — `AOS_FIELDS`.

    The values are bit-identical to `bulk_microphysics_tendencies` on the same points."""
    if not isinstance(scheme, Microphysics2Moment):
        raise TypeError("only Microphysics2Moment() is on this path")
    wr = _warm_rain(mp)
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    fam = _fam_of(rho)
    if fam is not wr.fam or not isinstance(tps, fam.thermo):
        raise TypeError("parameter float type does not match the state columns")
    flags = _abi.CMX_SB2006_LIMITED if wr.is_limited else 0
    r = _fields_call("cmx_sb2006_warm_rain_tendencies_fields", wr.c, tps, flags, cols, ("rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai"),
                     4, 8, out, aos, stream)
    return r if aos else WarmRainTendencies2M(*r, None, None)


def sb2006_process_rates(mp, tps, q_tot, q_lcl, q_rai, N_lcl, N_rai, rho, T, *, vel=SB2006VelType, vel_params=None, stream=None):
    """The individual SB2006 process rates over columns — the reference's SB2006_2M_kernel
    (test/gpu_tests.jl:220-235) + cond/evap (NonEq:117-140).  N_* are per m³ (CM2 convention).
    `vel_params` = a `cmx_rain_vel` struct with non-default fall-speed parameters (default: `parameters.rain_vel_params(FT)`)."""
    wr = _warm_rain(mp)
    cols = (q_tot, q_lcl, q_rai, N_lcl, N_rai, rho, T)
    ref = _check_cols(cols, ("q_tot", "q_lcl", "q_rai", "N_lcl", "N_rai", "rho", "T"))
    fam = _fam_of(ref)
    if fam is not wr.fam or not isinstance(tps, fam.thermo):
        raise TypeError("parameter float type does not match the state columns")
    vflag = _vel_flag(vel)
    outs = [torch.empty_like(ref) for _ in range(_abi.CMX_SB2006_NPROC)]
    if not vflag:
        outs[_abi.SB2006_PROCESS_COLUMNS.index("rain_vel_n")] = None
        outs[_abi.SB2006_PROCESS_COLUMNS.index("rain_vel_m")] = None
    arr = (C.c_void_p * _abi.CMX_SB2006_NPROC)(*[o.data_ptr() if o is not None else None for o in outs])
    flags = (_abi.CMX_SB2006_LIMITED if wr.is_limited else 0) | vflag
    velp = (vel_params if vel_params is not None else rain_vel_params(fam.sfx)) if vflag else None
    if velp is not None and not isinstance(velp, fam.rain_vel):
        raise TypeError("vel_params must be the cmx_rain_vel struct of the state's float type")
    _lib.call("cmx_sb2006_process_rates", fam, ref.device, C.byref(wr.c), C.byref(tps), C.byref(velp) if velp is not None else None, flags,
              ref.numel(), *[_ptr(t) for t in cols], arr, stream=stream)
    return SB2006ProcessRates(*outs)


def column_sums(cols, stream=None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Σ of each device column (double accumulation) → float64 tensor [len(cols)] on the device (≤ 16 columns).
    Building block of the optional diagnostic reduction; no communication here.  Deterministic: one launch over all
    columns into `workspace` (len(cols) × 1024 doubles, allocated here unless given), then a fixed-tree finish — bit-identical from run
    to run (include/cmx.h §3)."""
    cols = list(cols)
    if len(cols) > _abi.CMX_COLUMN_SUMS_MAX_COLS:
        raise ValueError(f"at most {_abi.CMX_COLUMN_SUMS_MAX_COLS} columns per call")
    ref = _check_cols(cols, [f"col{i}" for i in range(len(cols))])
    fam = _fam_of(ref)
    sums = torch.empty(len(cols), dtype=torch.float64, device=ref.device)
    need = len(cols) * _abi.CMX_COLUMN_SUMS_PARTIALS
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=ref.device)
    elif workspace.dtype != torch.float64 or workspace.device != ref.device or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError(f"workspace: a contiguous float64 device tensor of at least {need} elements")
    arr = (C.c_void_p * len(cols))(*[t.data_ptr() for t in cols])
    _lib.call("cmx_column_sums", fam, ref.device, len(cols), arr, ref.numel(), _ptr(sums), _ptr(workspace), stream=stream)
    return sums


CloudTerminalVelocity = namedtuple("CloudTerminalVelocity", ["vt_n", "vt_m"])


def cloud_terminal_velocity(pdf_c, vel, q_liq, rho, N_liq, *, stream=None) -> CloudTerminalVelocity:
    """`CM2.cloud_terminal_velocity.(Ref(pdf_c), Ref(vel), q_liq, ρₐ, N_liq)` (src/Microphysics2M.jl:647-664): number- and
    mass-weighted mean fall speeds of the cloud droplets; `pdf_c` = SB2006(FT).pdf_c, `vel` = StokesRegimeVelType(FT);
    N_liq per m³."""
    cols = (q_liq, rho, N_liq)
    ref = _check_cols(cols, ("q_liq", "rho", "N_liq"))
    fam = _fam_of(ref)
    if not isinstance(pdf_c, fam.cloud_pdf_sb2006) or not isinstance(vel, fam.stokes_vel):
        raise TypeError("parameter float type does not match the state columns")
    out = CloudTerminalVelocity(torch.empty_like(ref), torch.empty_like(ref))
    _lib.call("cmx_sb2006_cloud_terminal_velocity", fam, ref.device, C.byref(pdf_c), C.byref(vel), ref.numel(), *[_ptr(t) for t in cols],
              _ptr(out.vt_n), _ptr(out.vt_m), stream=stream)
    return out


ColumnTendencies2M = namedtuple("ColumnTendencies2M", ["dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt", "precip_flux"])


def column_tendencies_sedimentation(mp, tps, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, *, vel=SB2006VelType, vel_params=None, cloud_vel=None,
                                    want_precip_flux: bool = False, out: Optional[ColumnTendencies2M] = None,
                                    stream=None) -> ColumnTendencies2M:
    """SURVEY §8f-4 — the fused column step behind `cmx_sb2006_column_tendencies_sedimentation_*`: per column of `n_lev`
    contiguous levels (state tensors of shape (n_col, n_lev), level 0 = lowest)

        BMT.bulk_microphysics_tendencies(Microphysics2Moment(), mp, tps, ρ, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)   BMT:820-854
        CM2.rain_terminal_velocity(sb, vel, q_rai, ρ, ρ n_rai)  [+ CM2.cloud_terminal_velocity iff `cloud_vel`]     CM2:685-719, 647-664

    plus the host model's first-order upwind sedimentation flux divergence ∂χ/∂t += (F_{k+1} − F_k)/(ρ_k Δz_k), F = ρ χ w
    (the flux scheme is the host model's, not the reference's: include/cmx.h).  `inv_dz`: the n_lev values 1/Δz_k.
    `cloud_vel` = parameters.StokesRegimeVelType(FT) adds cloud-droplet sedimentation of q_lcl / n_lcl; `vel_params` = a `cmx_rain_vel` struct
    with non-default fall-speed parameters (default: `parameters.rain_vel_params(FT)`)."""
    wr = _warm_rain(mp)
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    ref = _check_cols(cols, ("rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai"))
    if ref.dim() != 2:
        raise ValueError("state columns must have shape (n_col, n_lev)")
    n_col, n_lev = ref.shape
    fam = _fam_of(ref)
    if fam is not wr.fam or not isinstance(tps, fam.thermo) or (cloud_vel is not None and not isinstance(cloud_vel, fam.stokes_vel)):
        raise TypeError("parameter float type does not match the state columns")
    if inv_dz.dtype != ref.dtype or inv_dz.device != ref.device or inv_dz.numel() != n_lev or not inv_dz.is_contiguous():
        raise ValueError("inv_dz must be a contiguous device vector of n_lev values of the state dtype")
    flag = _vel_flag(vel)
    if not flag:
        raise ValueError("the column step needs a rain fall-speed scheme (SB2006VelType or Chen2022VelTypeRain)")
    if out is None:
        out = ColumnTendencies2M(*[torch.empty_like(ref) for _ in range(4)],
                                 torch.empty(n_col, dtype=ref.dtype, device=ref.device) if want_precip_flux else None)
    else:
        _check_cols([ref, *out[:4]], ["rho", *ColumnTendencies2M._fields[:4]])
    flags = (_abi.CMX_SB2006_LIMITED if wr.is_limited else 0) | flag
    velp = vel_params if vel_params is not None else rain_vel_params(fam.sfx)
    if not isinstance(velp, fam.rain_vel):
        raise TypeError("vel_params must be the cmx_rain_vel struct of the state's float type")
    _lib.call("cmx_sb2006_column_tendencies_sedimentation", fam, ref.device, C.byref(wr.c), C.byref(tps), C.byref(velp),
              C.byref(cloud_vel) if cloud_vel is not None else None, flags, n_col, n_lev, _ptr(inv_dz), *[_ptr(t) for t in cols],
              *[_ptr(t) for t in out[:4]], _ptr(out.precip_flux), stream=stream)
    return out


ColumnJvp2M = namedtuple("ColumnJvp2M", ["jvp", "jvp_precip", "tendencies", "precip_flux"])
ColumnVjp2M = namedtuple("ColumnVjp2M", ["grad", "tendencies", "precip_flux", "wrt"])


def _column_products_head(mp, tps, inv_dz, cols, vel, vel_params, cloud_vel):
    """The checks of `column_tendencies_sedimentation` for the two products with its Jacobian: (reference column, float family, the ABI arguments from the
    parameter structs through n_rai)."""
    wr = _warm_rain(mp)
    ref = _check_cols(cols, _NAMES_2M)
    if ref.dim() != 2:
        raise ValueError("state columns must have shape (n_col, n_lev)")
    n_col, n_lev = ref.shape
    fam = _fam_of(ref)
    if fam is not wr.fam or not isinstance(tps, fam.thermo) or (cloud_vel is not None and not isinstance(cloud_vel, fam.stokes_vel)):
        raise TypeError("parameter float type does not match the state columns")
    if inv_dz.dtype != ref.dtype or inv_dz.device != ref.device or inv_dz.numel() != n_lev or not inv_dz.is_contiguous():
        raise ValueError("inv_dz must be a contiguous device vector of n_lev values of the state dtype")
    flag = _vel_flag(vel)
    if not flag:
        raise ValueError("the column step needs a rain fall-speed scheme (SB2006VelType or Chen2022VelTypeRain)")
    velp = vel_params if vel_params is not None else rain_vel_params(fam.sfx)
    if not isinstance(velp, fam.rain_vel):
        raise TypeError("vel_params must be the cmx_rain_vel struct of the state's float type")
    flags = (_abi.CMX_SB2006_LIMITED if wr.is_limited else 0) | flag
    keep = (wr, velp)      # the structs the pointers below refer to
    return ref, fam, keep, (C.byref(wr.c), C.byref(tps), C.byref(velp), C.byref(cloud_vel) if cloud_vel is not None else None, flags, n_col, n_lev,
                            _ptr(inv_dz), *[_ptr(t) for t in cols])


def _column_primal_out(ref, with_tendencies):
    if not with_tendencies:
        return None, None
    return torch.empty((4, *ref.shape), dtype=ref.dtype, device=ref.device), torch.empty(ref.shape[0], dtype=ref.dtype, device=ref.device)


def column_jvp_2m(mp, tps, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, tangents, with_tendencies=False, *, vel=SB2006VelType, vel_params=None,
                  cloud_vel=None, stream=None) -> ColumnJvp2M:
    """J v of `column_tendencies_sedimentation` — the four tendencies WITH the upwind flux divergence of the falling species — and of its precipitation flux,
    behind `cmx_sb2006_column_jvp_*` (include/cmx.h §25): the matvec of a Newton–Krylov solver that treats microphysics and sedimentation implicitly
    together.  One launch; ρ and `inv_dz` are held fixed.

    State columns of shape (n_col, n_lev), `inv_dz`, `vel`, `vel_params`, `cloud_vel` as for `column_tendencies_sedimentation`.  `tangents`: dict name ->
    tensor of the state's shape over `JACOBIAN_WRT`; a missing name is a zero tangent.  Returns `ColumnJvp2M(jvp, jvp_precip, tendencies, precip_flux)`:
    `jvp` of shape (4, n_col, n_lev) in the order of `JACOBIAN_OUTPUTS`, `jvp_precip` (n_col,); with `with_tendencies=True` also `tendencies`
    (4, n_col, n_lev) and `precip_flux` (n_col,), bit-identical to `column_tendencies_sedimentation`, else None.  Asynchronous on `stream`."""
    if not isinstance(tangents, dict):
        raise TypeError("tangents must be a dict: name of a differentiable input -> tensor")
    _check_wrt(tangents.keys(), JACOBIAN_WRT, "tangents")
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    ref, fam, keep, head = _column_products_head(mp, tps, inv_dz, cols, vel, vel_params, cloud_vel)
    given = [(k, v) for k, v in tangents.items() if v is not None]
    if given:
        _check_cols([ref] + [v for _, v in given], ["rho"] + [f"tangent of {k}" for k, _ in given])
    jvp = torch.empty((4, *ref.shape), dtype=ref.dtype, device=ref.device)
    jvp_precip = torch.empty(ref.shape[0], dtype=ref.dtype, device=ref.device)
    tend, precip = _column_primal_out(ref, with_tendencies)
    _lib.call("cmx_sb2006_column_jvp", fam, ref.device, *head, _table([tangents.get(name) for name in JACOBIAN_WRT]), _table([jvp[o] for o in range(4)]),
              _ptr(jvp_precip), _table([tend[o] for o in range(4)]) if tend is not None else None, _ptr(precip), stream=stream)
    return ColumnJvp2M(jvp, jvp_precip, tend, precip)


def column_vjp_2m(mp, tps, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, cotangents, cot_precip=None, wrt=JACOBIAN_WRT, with_tendencies=False, *,
                  vel=SB2006VelType, vel_params=None, cloud_vel=None, stream=None) -> ColumnVjp2M:
    """Jᵀḡ of `column_tendencies_sedimentation` and its precipitation flux behind `cmx_sb2006_column_vjp_*` (include/cmx.h §25): the gradient of
    Σ ḡ·tendencies + Σ p̄·precip_flux with respect to the inputs `wrt` — what `loss(precip_flux).backward()` needs (cmx.autograd).  One launch.

    `cotangents`: a sequence of 4 tensors of the state's shape or None in the order of `JACOBIAN_OUTPUTS` (None: that output is not part of the sum);
    `cot_precip`: a tensor of n_col values or None.  `wrt`: any subset of `JACOBIAN_WRT` in any order.  Returns `ColumnVjp2M(grad, tendencies, precip_flux,
    wrt)`: `grad` of shape (len(wrt), n_col, n_lev) — a cotangent at level k reaches the gradients at levels k and k + 1 of its column; a gradient does not
    depend on which others are requested.  `tendencies`, `precip_flux` and the other arguments as for `column_jvp_2m`."""
    wrt = _check_wrt(wrt, JACOBIAN_WRT)
    cotangents = list(cotangents)
    if len(cotangents) != 4:
        raise ValueError("cotangents: 4 tensors (or None) expected, one per output")
    if not wrt and not with_tendencies:
        raise ValueError("nothing to compute: wrt is empty and with_tendencies is False")
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    ref, fam, keep, head = _column_products_head(mp, tps, inv_dz, cols, vel, vel_params, cloud_vel)
    given = [(o, g) for o, g in enumerate(cotangents) if g is not None]
    if given:
        _check_cols([ref] + [g for _, g in given], ["rho"] + [f"cotangent {o}" for o, _ in given])
    if cot_precip is not None and (cot_precip.dtype != ref.dtype or cot_precip.device != ref.device or cot_precip.shape != (ref.shape[0],)
                                   or not cot_precip.is_contiguous()):
        raise ValueError("cot_precip must be a contiguous device vector of n_col values of the state dtype")
    grad = torch.empty((len(wrt), *ref.shape), dtype=ref.dtype, device=ref.device)
    grads = [None] * len(JACOBIAN_WRT)
    for k, name in enumerate(wrt):
        grads[JACOBIAN_WRT.index(name)] = grad[k]
    tend, precip = _column_primal_out(ref, with_tendencies)
    _lib.call("cmx_sb2006_column_vjp", fam, ref.device, *head, _table(cotangents), _ptr(cot_precip), _table(grads),
              _table([tend[o] for o in range(4)]) if tend is not None else None, _ptr(precip), stream=stream)
    return ColumnVjp2M(grad, tend, precip, wrt)


ColumnParamJvp2M = namedtuple("ColumnParamJvp2M", ["jvp", "jvp_precip", "tendencies", "precip_flux"])
ColumnParamVjp2M = namedtuple("ColumnParamVjp2M", ["grad", "tendencies", "precip_flux", "wrt"])


def _column_param_directions(mp, fam, directions, vel_params, cloud_vel):
    """The four direction tables of include/cmx.h §26 from a sequence whose members are {ClimaParams name: weight} mappings or the 4-tuples of
    `parameters.column_parameter_direction`."""
    wr = _warm_rain(mp)
    quads = [column_parameter_direction(wr, d, vel_params, cloud_vel) if isinstance(d, dict) else tuple(d) for d in directions]
    if not quads:
        raise ValueError("directions: at least one direction expected")
    types = (fam.warm_rain_2m, fam.thermo, fam.rain_vel, fam.stokes_vel)
    for q in quads:
        if len(q) != 4 or not all(isinstance(a, t) for a, t in zip(q, types)):
            raise TypeError("directions: (d_warm_rain, d_thermo, d_rain_vel, d_stokes_vel) structs of the state's float type, or {name: weight} mappings")
    return [(t * len(quads))(*[q[k] for q in quads]) for k, t in enumerate(types)]


def column_param_jvp_2m(mp, tps, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, directions, with_tendencies=False, *, vel=SB2006VelType, vel_params=None,
                        cloud_vel=None, stream=None) -> ColumnParamJvp2M:
    """J_θ·δθ of `column_tendencies_sedimentation` — the four tendencies with the flux divergence of the falling species — and of its precipitation flux with
    respect to the scheme's PARAMETERS, the fall-speed parameters included, behind `cmx_sb2006_column_param_jvp_*` (include/cmx.h §26).  The state, ρ and
    `inv_dz` are held fixed.

    Arguments as for `column_jvp_2m`; `directions`: a sequence of {ClimaParams name: weight} mappings (`parameters.COLUMN_2M_DIRECTION_FIELDS` has the names)
    or of the 4-tuples of `parameters.column_parameter_direction`.  Returns `ColumnParamJvp2M(jvp, jvp_precip, tendencies, precip_flux)`: `jvp` of shape
    (len(directions), 4, n_col, n_lev), `jvp_precip` (len(directions), n_col); a column does not depend on which other directions are in the call.  The
    Chen-2022 table is held fixed: a direction on it raises CmxStatusError (CMX_ERR_UNSUPPORTED).  Asynchronous on `stream`."""
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    ref, fam, keep, head = _column_products_head(mp, tps, inv_dz, cols, vel, vel_params, cloud_vel)
    tables = _column_param_directions(mp, fam, directions, keep[1], cloud_vel)
    ndir = len(tables[0])
    jvp = torch.empty((ndir, 4, *ref.shape), dtype=ref.dtype, device=ref.device)
    jvp_precip = torch.empty((ndir, ref.shape[0]), dtype=ref.dtype, device=ref.device)
    tend, precip = _column_primal_out(ref, with_tendencies)
    for d0 in range(0, ndir, _abi.CMX_PARAM_MAX_DIRS):
        nd = min(_abi.CMX_PARAM_MAX_DIRS, ndir - d0)
        first = d0 == 0 and tend is not None
        _lib.call("cmx_sb2006_column_param_jvp", fam, ref.device, *head, nd, *[C.byref(t[d0]) for t in tables],
                  _table([jvp[d, o] for d in range(d0, d0 + nd) for o in range(4)]), _table([jvp_precip[d] for d in range(d0, d0 + nd)]),
                  _table([tend[o] for o in range(4)]) if first else None, _ptr(precip) if first else None, stream=stream)
    return ColumnParamJvp2M(jvp, jvp_precip, tend, precip)


def column_param_vjp_2m(mp, tps, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, cotangents, cot_precip=None, wrt=(), with_tendencies=False, *,
                        vel=SB2006VelType, vel_params=None, cloud_vel=None, stream=None) -> ColumnParamVjp2M:
    """The gradient of Σ ḡ·tendencies + Σ p̄·precip_flux of `column_tendencies_sedimentation` with respect to the PARAMETERS behind
    `cmx_sb2006_column_param_vjp_*` (include/cmx.h §26): what `loss(precip_flux).backward()` needs to reach `theta` (cmx.autograd).

    `cotangents`, `cot_precip` as for `column_vjp_2m`; `wrt`: ClimaParams names (one-hot directions) or directions as for `column_param_jvp_2m`.  Returns
    `ColumnParamVjp2M(grad, tendencies, precip_flux, wrt)`: `grad` a float64 tensor of len(wrt) values on the state's device — a fixed-order reduction,
    bit-identical from run to run."""
    wrt = tuple(wrt)
    cotangents = list(cotangents)
    if len(cotangents) != 4:
        raise ValueError("cotangents: 4 tensors (or None) expected, one per output")
    cols = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
    ref, fam, keep, head = _column_products_head(mp, tps, inv_dz, cols, vel, vel_params, cloud_vel)
    tables = _column_param_directions(mp, fam, [{w: 1.0} if isinstance(w, str) else w for w in wrt], keep[1], cloud_vel)
    given = [(o, g) for o, g in enumerate(cotangents) if g is not None]
    if given:
        _check_cols([ref] + [g for _, g in given], ["rho"] + [f"cotangent {o}" for o, _ in given])
    if cot_precip is not None and (cot_precip.dtype != ref.dtype or cot_precip.device != ref.device or cot_precip.shape != (ref.shape[0],)
                                   or not cot_precip.is_contiguous()):
        raise ValueError("cot_precip must be a contiguous device vector of n_col values of the state dtype")
    ndir = len(tables[0])
    grad = torch.empty(ndir, dtype=torch.float64, device=ref.device)
    workspace = torch.empty(min(ndir, _abi.CMX_PARAM_MAX_DIRS) * _abi.CMX_PARAM_VJP_PARTIALS, dtype=torch.float64, device=ref.device)
    tend, precip = _column_primal_out(ref, with_tendencies)
    for d0 in range(0, ndir, _abi.CMX_PARAM_MAX_DIRS):
        nd = min(_abi.CMX_PARAM_MAX_DIRS, ndir - d0)
        first = d0 == 0 and tend is not None
        _lib.call("cmx_sb2006_column_param_vjp", fam, ref.device, *head, _table(cotangents), _ptr(cot_precip), nd, *[C.byref(t[d0]) for t in tables],
                  _ptr(grad[d0:]), _ptr(workspace), _table([tend[o] for o in range(4)]) if first else None, _ptr(precip) if first else None, stream=stream)
    return ColumnParamVjp2M(grad, tend, precip, wrt)


def _column_implicit_2m(entry, mp, tps, inv_dz, cols, dt, nsub, nonnegative, vel, vel_params, cloud_vel, want_precip_flux, out, stream):
    """The checks and the call of the two 2-moment column steps that take the implicit average as tendency (include/cmx.h §(20), §(21)): same arguments."""
    wr = _warm_rain(mp)
    dt, nsub = _check_step(dt, nsub)
    ref = _check_cols(cols, _NAMES_2M)
    if ref.dim() != 2:
        raise ValueError("state columns must have shape (n_col, n_lev)")
    n_col, n_lev = ref.shape
    fam = _fam_of(ref)
    if fam is not wr.fam or not isinstance(tps, fam.thermo) or (cloud_vel is not None and not isinstance(cloud_vel, fam.stokes_vel)):
        raise TypeError("parameter float type does not match the state columns")
    _check_step_normal(dt, nsub, ref.dtype)
    if inv_dz.dtype != ref.dtype or inv_dz.device != ref.device or inv_dz.numel() != n_lev or not inv_dz.is_contiguous():
        raise ValueError("inv_dz must be a contiguous device vector of n_lev values of the state dtype")
    flag = _vel_flag(vel)
    if not flag:
        raise ValueError("the column step needs a rain fall-speed scheme (SB2006VelType or Chen2022VelTypeRain)")
    if out is None:
        out = ColumnTendencies2M(*[torch.empty_like(ref) for _ in range(4)],
                                 torch.empty(n_col, dtype=ref.dtype, device=ref.device) if want_precip_flux else None)
    else:
        _check_cols([ref, *out[:4]], ["rho", *ColumnTendencies2M._fields[:4]])
        state = {c.data_ptr() for c in cols}
        if any(o.data_ptr() in state for o in out[:4]):
            raise ValueError("an output column must not be a state column: this step is not in place")
    flags = (_abi.CMX_SB2006_LIMITED if wr.is_limited else 0) | flag
    velp = vel_params if vel_params is not None else rain_vel_params(fam.sfx)
    if not isinstance(velp, fam.rain_vel):
        raise TypeError("vel_params must be the cmx_rain_vel struct of the state's float type")
    _lib.call(entry, fam, ref.device, C.byref(wr.c), C.byref(tps), C.byref(velp),
              C.byref(cloud_vel) if cloud_vel is not None else None, flags, dt, nsub, _abi.CMX_STEP_NONNEGATIVE if nonnegative else 0, n_col, n_lev,
              _ptr(inv_dz), *[_ptr(t) for t in cols], *[_ptr(t) for t in out[:4]], _ptr(out.precip_flux), stream=stream)
    return out


def column_implicit_average_sedimentation_2m(mp, tps, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dt, nsub=1, nonnegative=True, *, vel=SB2006VelType,
                                             vel_params=None, cloud_vel=None, want_precip_flux: bool = False, out: Optional[ColumnTendencies2M] = None,
                                             stream=None) -> ColumnTendencies2M:
    """The 2-moment column step with the sub-stepped implicit average as tendency operator (`cmx_sb2006_column_implicit_average_sedimentation_*`): per point
    the average tendency of `warm_rain_implicit_average_2m(…, dt, nsub, nonnegative)` — bit for bit — plus, in the same kernel, the first-order upwind
    sedimentation flux divergence of `column_tendencies_sedimentation` with the fluxes of the INITIAL state (sedimentation stays explicit).  A stable
    large-`dt` column step in one launch; include/cmx.h §(20) has the definition.

    State tensors of shape (n_col, n_lev), level 0 lowest, contiguous (a transposed view is refused); `inv_dz`, `vel`, `vel_params`, `cloud_vel`,
    `want_precip_flux` as for `column_tendencies_sedimentation`; `dt`, `nsub`, `nonnegative` as for `warm_rain_implicit_average_2m`.  `out=` provides the
    outputs; an output must NOT be a state tensor (another workgroup reads the point above).  No autograd.  Asynchronous on `stream`."""
    return _column_implicit_2m("cmx_sb2006_column_implicit_average_sedimentation", mp, tps, inv_dz, (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai), dt, nsub,
                               nonnegative, vel, vel_params, cloud_vel, want_precip_flux, out, stream)


def column_implicit_step_2m(mp, tps, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dt, nsub=1, nonnegative=True, *, vel=SB2006VelType,
                            vel_params=None, cloud_vel=None, want_precip_flux: bool = False, out: Optional[ColumnTendencies2M] = None,
                            stream=None) -> ColumnTendencies2M:
    """The 2-moment column step that is stable and positive at any Courant number Δt·w/Δz (`cmx_sb2006_column_implicit_step_*`): the average tendency of
    `warm_rain_implicit_average_2m(…, dt, nsub, nonnegative)` per point — bit for bit — and, in the same kernel, BACKWARD-EULER first-order upwind
    sedimentation, a top-down recurrence along each column with the fall speeds of the initial state.  Where `column_implicit_average_sedimentation_2m`
    (explicit fluxes) needs Δt·w/Δz ≤ 1, this step needs no sub-cycling.  `precip_flux` is the flux that leaves the column DURING the step (G_0, not the
    initial F_0): the column budget closes.  include/cmx.h §(21) has the definition.

    Arguments, result, `out=` and the checks are those of `column_implicit_average_sedimentation_2m`; an output must NOT be a state tensor.  No autograd.
    Asynchronous on `stream`."""
    return _column_implicit_2m("cmx_sb2006_column_implicit_step", mp, tps, inv_dz, (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai), dt, nsub, nonnegative, vel,
                               vel_params, cloud_vel, want_precip_flux, out, stream)


ColumnTendencies2MP3 = namedtuple(
    "ColumnTendencies2MP3",
    ["dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt", "dq_ice_dt", "dn_ice_dt", "dq_rim_dt", "db_rim_dt", "log_lambda", "v_ice_n", "v_ice_m",
     "precip_rai", "precip_ice"])

# the rain fall-speed scheme in the flag word of the 2M + P3 column step (bits 1 and 2 are P3 flags there: include/cmx.h (9b))
_P3COL_VEL = {_abi.CMX_VEL_SB2006: _abi.CMX_P3COL_VEL_SB2006, _abi.CMX_VEL_CHEN2022: _abi.CMX_P3COL_VEL_CHEN2022}


def column_tendencies_sedimentation_2m_p3(mp, tps, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, *,
                                          log_lambda_guess=None, inpc_log_shift=None, vel=SB2006VelType, vel_params=None, cloud_vel=None,
                                          p: float = 1e-6, brent_iters: int = 0, aspect_ratio: bool = True, want_precip_flux: bool = False,
                                          out: Optional[ColumnTendencies2MP3] = None, stream=None) -> ColumnTendencies2MP3:
    """The 2M + P3 column step behind `cmx_mp2m_p3_column_tendencies_sedimentation_*` — one call per time step of a mixed-phase host model.
    Per column of `n_lev` contiguous levels (state tensors of shape (n_col, n_lev), level 0 = lowest), in this order:

        p3_shape_and_terminal_velocities(mp.ice.scheme…, ρ, ρ q_ice, ρ n_ice, ρ q_rim, ρ b_rim; log_lambda_guess, brent_iters, p, quad = mp.ice's)
        bulk_microphysics_tendencies(Microphysics2Moment(), mp, tps, ρ, …, b_rim, log_lambda, inpc_log_shift)            BMT:898-1083
        CM2.rain_terminal_velocity(sb, vel, q_rai, ρ, ρ n_rai)  [+ CM2.cloud_terminal_velocity iff `cloud_vel`]          CM2:685-719, 647-664

    plus the host model's first-order upwind sedimentation flux divergence ∂χ/∂t += (F_{k+1} − F_k)/(ρ_k Δz_k), F = ρ χ w, of q_rai, n_rai
    (rain speeds), q_ice, q_rim, b_rim (v_ice_m), n_ice (v_ice_n) and — with `cloud_vel` — q_lcl, n_lcl (the flux scheme is the host model's,
    not the reference's: include/cmx.h).  `inv_dz`: the n_lev values 1/Δz_k.  Returns `ColumnTendencies2MP3`: the eight tendencies,
    `log_lambda` (cache it: it is the next step's `log_lambda_guess`), the ice fall speeds, and — `want_precip_flux` — the surface
    fluxes of q_rai and q_ice per column.  Points without ice: log λ = −Inf, speeds 0."""
    return _column_2m_p3("cmx_mp2m_p3_column_tendencies_sedimentation", None, mp, tps, inv_dz, (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim),
                         log_lambda_guess, inpc_log_shift, vel, vel_params, cloud_vel, p, brent_iters, aspect_ratio, want_precip_flux, out, stream)


def _column_2m_p3(entry, dt, mp, tps, inv_dz, cols, log_lambda_guess, inpc_log_shift, vel, vel_params, cloud_vel, p, brent_iters, aspect_ratio,
                  want_precip_flux, out, stream):
    """The checks and the call of the two 2M + P3 column steps (include/cmx.h (9b), §(24)): the same arguments; `dt`: None for (9b), else
    the step of §(24), judged last, as the C entry does."""
    if not (isinstance(mp, Microphysics2MParams) and mp.ice is not None):
        raise TypeError("mp must be Microphysics2MParams(FT, with_ice=True)")
    names = ("rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai", "q_ice", "n_ice", "q_rim", "b_rim")
    ref = _check_cols(cols, names)
    if ref.dim() != 2:
        raise ValueError("state columns must have shape (n_col, n_lev)")
    n_col, n_lev = ref.shape
    fam = _fam_of(ref)
    if fam is not mp.fam or fam is not mp.ice.fam or not isinstance(tps, fam.thermo) or \
            (cloud_vel is not None and not isinstance(cloud_vel, fam.stokes_vel)):
        raise TypeError("parameter float type does not match the state columns")
    if mp.ice.is_limited != mp.warm_rain.is_limited:
        raise ValueError("warm_rain and ice must use the same rain PSD variant (is_limited)")
    if inv_dz.dtype != ref.dtype or inv_dz.device != ref.device or inv_dz.numel() != n_lev or not inv_dz.is_contiguous():
        raise ValueError("inv_dz must be a contiguous device vector of n_lev values of the state dtype")
    flag = _vel_flag(vel)
    if not flag:
        raise ValueError("the column step needs a rain fall-speed scheme (SB2006VelType or Chen2022VelTypeRain)")
    for t, nm in ((log_lambda_guess, "log_lambda_guess"), (inpc_log_shift, "inpc_log_shift")):
        if t is not None:
            _check_cols([ref, t], ["rho", nm])
    if out is None:
        mk = lambda: torch.empty_like(ref)  # noqa: E731
        pf = lambda: torch.empty(n_col, dtype=ref.dtype, device=ref.device) if want_precip_flux else None  # noqa: E731
        out = ColumnTendencies2MP3(*[mk() for _ in range(11)], pf(), pf())
    else:
        _check_cols([ref, *out[:11]], ["rho", *ColumnTendencies2MP3._fields[:11]])
        for t, nm in zip(out[11:], ColumnTendencies2MP3._fields[11:]):
            if t is not None and (t.dtype != ref.dtype or t.device != ref.device or t.numel() != n_col or not t.is_contiguous()):
                raise ValueError(f"{nm} must be a contiguous device vector of n_col values of the state dtype")
    velp = vel_params if vel_params is not None else rain_vel_params(fam.sfx)
    if not isinstance(velp, fam.rain_vel):
        raise TypeError("vel_params must be the cmx_rain_vel struct of the state's float type")
    after_p = ()
    if dt is not None:
        dt = float(dt)
        if not (math.isfinite(dt) and dt >= 0.0):
            raise ValueError("dt must be finite and >= 0")
        after_p = (dt,)
    flags = mp.ice.flags | (0 if aspect_ratio else _abi.CMX_P3_NO_ASPECT_RATIO) | _P3COL_VEL[flag]
    in_p = (C.c_void_p * 13)(*[t.data_ptr() for t in cols], log_lambda_guess.data_ptr() if log_lambda_guess is not None else None,
                             inpc_log_shift.data_ptr() if inpc_log_shift is not None else None)
    out_p = (C.c_void_p * 8)(*[t.data_ptr() for t in out[:8]])
    _lib.call(entry, fam, ref.device, C.byref(mp.warm_rain.c), C.byref(mp.ice.c), C.byref(tps), C.byref(velp),
              C.byref(cloud_vel) if cloud_vel is not None else None, flags, int(brent_iters), p, *after_p, n_col, n_lev, _ptr(inv_dz), in_p, out_p,
              _ptr(out.log_lambda), _ptr(out.v_ice_n), _ptr(out.v_ice_m), _ptr(out.precip_rai), _ptr(out.precip_ice), stream=stream)
    return out


def column_implicit_sedimentation_2m_p3(mp, tps, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, dt, *,
                                        log_lambda_guess=None, inpc_log_shift=None, vel=SB2006VelType, vel_params=None, cloud_vel=None,
                                        p: float = 1e-6, brent_iters: int = 0, aspect_ratio: bool = True, want_precip_flux: bool = False,
                                        out: Optional[ColumnTendencies2MP3] = None, stream=None) -> ColumnTendencies2MP3:
    """`column_tendencies_sedimentation_2m_p3` with IMPLICIT sedimentation, behind `cmx_mp2m_p3_column_implicit_sedimentation_*`: the shape solve, the ice fall
    speeds and the eight tendencies are those of that step (the same launches, the same bits), and backward-Euler first-order upwind sedimentation — a top-down
    recurrence along each column with the fall speeds of the initial state — stands in the place of the explicit flux divergence.  Stable at any Courant
    number Δt·w/Δz, where the explicit step needs ≤ 1 (rimed ice at 5–9 m/s, rain at up to 12 m/s): no sub-cycling.  `precip_rai` and `precip_ice` are the
    fluxes that leave the column DURING the step (G_0, not the initial F_0): the column budget closes.  include/cmx.h §(24) has the definition.

    `dt`: the step [s], finite and ≥ 0 (at 0 the result is that of `column_tendencies_sedimentation_2m_p3`).  Every other argument, the keywords, the checks
    and the result are those of `column_tendencies_sedimentation_2m_p3`.  No autograd.  Asynchronous on `stream`."""
    if dt is None:
        raise TypeError("dt must be a number")
    return _column_2m_p3("cmx_mp2m_p3_column_implicit_sedimentation", dt, mp, tps, inv_dz, (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim),
                         log_lambda_guess, inpc_log_shift, vel, vel_params, cloud_vel, p, brent_iters, aspect_ratio, want_precip_flux, out, stream)


_SCHEMES_2M = {"KK2000": _abi.CMX_2M_KK2000, "B1994": _abi.CMX_2M_B1994, "TC1980": _abi.CMX_2M_TC1980, "LD2004": _abi.CMX_2M_LD2004}
CloudToRain2M = namedtuple("CloudToRain2M", ["acnv", "accr"])


def bulk_2m_cloud_to_rain(schemes, scheme: str, q_lcl, rho, N_d=None, q_rai=None, *, smooth_transition=False,
                          stream=None) -> CloudToRain2M:
    """`CM2.conv_q_lcl_to_q_rai.(Ref(scheme), q_lcl, ρ, N_d[, smooth_transition])` (→ `acnv`, needs N_d [1/m³]) and
    `CM2.accretion.(Ref(scheme), q_lcl, q_rai, ρ)` (→ `accr`, needs q_rai) for scheme ∈ KK2000 | B1994 | TC1980 | LD2004
    (src/Microphysics2M.jl:920-1003); `schemes` = parameters.Bulk2MSchemes(FT)."""
    if scheme not in _SCHEMES_2M:
        raise ValueError(f"scheme must be one of {sorted(_SCHEMES_2M)}")
    if scheme == "LD2004" and q_rai is not None:
        raise ValueError("LD2004 has no accretion parameterization")
    cols = [c for c in (q_lcl, rho, N_d, q_rai) if c is not None]
    ref = _check_cols(cols, ["q_lcl", "rho", "N_d", "q_rai"][:len(cols)])
    fam = _fam_of(ref)
    if not isinstance(schemes, fam.bulk_2m_schemes):
        raise TypeError("parameter float type does not match the state columns")
    if N_d is None and q_rai is None:
        raise ValueError("pass N_d (autoconversion) and / or q_rai (accretion)")
    acnv = torch.empty_like(ref) if N_d is not None else None
    accr = torch.empty_like(ref) if q_rai is not None else None
    flags = _SCHEMES_2M[scheme] | (_abi.CMX_2M_SMOOTH_TRANSITION if smooth_transition else 0)
    _lib.call("cmx_bulk_2m_cloud_to_rain", fam, ref.device, C.byref(schemes), flags, ref.numel(), _ptr(q_lcl), _ptr(q_rai), _ptr(rho), _ptr(N_d),
              _ptr(acnv), _ptr(accr), stream=stream)
    return CloudToRain2M(acnv, accr)
