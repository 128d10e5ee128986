"""One-moment (Marshall–Palmer) scheme over columns — host-side mirror of the 1M entry of
`CloudMicrophysics.BulkMicrophysicsTendencies` and of `CloudMicrophysics.Microphysics1M.terminal_velocity`
(include/cmx.h §5).

Reference broadcasts being replaced:

    BMT.bulk_microphysics_tendencies.(Ref(BMT.Instantaneous()), Ref(BMT.Microphysics1Moment()), Ref(mp), Ref(tps),
                                      ρ, T, q_tot, q_lcl, q_icl, q_rai, q_sno)        # BMT:505-514
    @. w = CM1.terminal_velocity(rain, vel, ρ, q)                                      # test/gpu_clima_core_test.jl:39-42
    @. w = CM1.terminal_velocity(snow, Ch2022.large_ice, ρ, q, CM1.Oblate())          # src/Microphysics1M.jl:299-324
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _abi, _lib
from ._cols import _check_cols, _fam_of, _fields_call, _ptr
from ._jacobian import _check_step, _check_step_normal, _check_wrt, _implicit, _implicit_average, _jacobian, _jvp, _param_jvp, _param_vjp, _table, _vjp
from .parameters import Chen2022VelTypeRain, Microphysics1MParams, column_parameter_direction_1m


class AbstractSnowShape:
    """CM1.AbstractSnowShape — snow shape of the Chen-2022 snow fall speed (src/Microphysics1M.jl:66-68)."""
    _shape = _abi.CMX_SNOW_SHAPE_ASPR
    _column_bit = 0


class Oblate(AbstractSnowShape):
    """CM1.Oblate — oblate snow: ϕ(r) = 3√π m(r) / (4 ρᵢ a(r)^{3/2}), κ = 1/3 (CM1.aspect_ratio_coeffs, CM1:155-181)."""
    _shape = _abi.CMX_SNOW_SHAPE_OBLATE
    _column_bit = _abi.CMX_1M_SED_SNOW_OBLATE


class Prolate(AbstractSnowShape):
    """CM1.Prolate — prolate snow: ϕ(r) = 16 ρᵢ² a(r)³ / (9π m(r)²), κ = −1/6 (CM1:183-195)."""
    _shape = _abi.CMX_SNOW_SHAPE_PROLATE
    _column_bit = _abi.CMX_1M_SED_SNOW_PROLATE


def _shape_of(snow_shape):
    if snow_shape is None:
        return None
    if not isinstance(snow_shape, (Oblate, Prolate)):
        raise TypeError(f"snow_shape must be None, Oblate() or Prolate(), got {type(snow_shape).__name__}")
    return snow_shape


class Microphysics1Moment:
    """BMT.Microphysics1Moment — scheme tag (src/BulkMicrophysicsTendencies.jl:52-56)."""


class Instantaneous:
    """BMT.Instantaneous — tendency mode tag: raw point-wise tendencies (BMT:84-90)."""


class LinearizedAverage:
    """BMT.LinearizedAverage — tendency mode tag: average tendencies over Δt from `nsub` linearized implicit substeps
    (BMT:96-115, 572-632).  `bulk_microphysics_tendencies_1m(LinearizedAverage(), scheme, mp, tps, …, dt, nsub)`.
    `q_min` = TD.Parameters.q_min(tps), the donor floor of the linearization (parameters.DEFAULT_PARAMETERS
    "specific_humidity_minimum"; not pinned by any reference test)."""


Tendencies1M = namedtuple("Tendencies1M", ["dq_lcl_dt", "dq_icl_dt", "dq_rai_dt", "dq_sno_dt"])
SourceTerms1M = namedtuple("SourceTerms1M", _abi.MP1M_SOURCE_COLUMNS)
TerminalVelocities1M = namedtuple("TerminalVelocities1M", ["vt_rai_blk1m", "vt_sno_blk1m", "vt_rai_chen"])

_NAMES = ("rho", "T", "q_tot", "q_lcl", "q_icl", "q_rai", "q_sno")


def _prep(mp, tps, cols):
    if not isinstance(mp, Microphysics1MParams):
        raise TypeError("mp must be Microphysics1MParams")
    ref = _check_cols(cols, _NAMES)
    fam = _fam_of(ref)
    if fam is not mp.fam or not isinstance(tps, fam.thermo):
        raise TypeError("parameter float type does not match the state columns")
    return ref, fam


def bulk_microphysics_tendencies_1m(mode, scheme, mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, dt=None, nsub=1, *,
                                    q_min=None, out=None, stream=None) -> Tendencies1M:
    """1-moment tendencies over columns — Instantaneous mode (BMT:505-514 → :141-252) or, with `dt` [, `nsub`],
    LinearizedAverage mode (BMT:572-632)."""
    if not isinstance(scheme, Microphysics1Moment) or not isinstance(mode, (Instantaneous, LinearizedAverage)):
        raise TypeError("mode must be Instantaneous() or LinearizedAverage() and scheme Microphysics1Moment()")
    cols = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    ref, fam = _prep(mp, tps, cols)
    if out is None:
        out = Tendencies1M(*[torch.empty_like(ref) for _ in range(4)])
    else:
        _check_cols([ref] + list(out), ["rho"] + ["out"] * 4)
    if isinstance(mode, LinearizedAverage):
        if dt is None or not dt > 0 or int(nsub) < 1:
            raise ValueError("LinearizedAverage needs dt > 0 and nsub >= 1")
        if q_min is None:
            from .parameters import DEFAULT_PARAMETERS
            q_min = DEFAULT_PARAMETERS["specific_humidity_minimum"]
        _lib.call("cmx_mp1m_linearized_average", fam, ref.device, C.byref(mp.c), C.byref(tps), mp.flags, q_min, dt, int(nsub), ref.numel(),
                  *[_ptr(t) for t in cols], *[_ptr(o) for o in out], stream=stream)
    else:
        if dt is not None:
            raise TypeError("Instantaneous() takes no dt")
        _lib.call("cmx_mp1m_tendencies", fam, ref.device, C.byref(mp.c), C.byref(tps), mp.flags, ref.numel(), *[_ptr(t) for t in cols],
                  *[_ptr(o) for o in out], stream=stream)
    return out


Jacobian1M = namedtuple("Jacobian1M", ["jac", "tendencies", "wrt"])

JACOBIAN_OUTPUTS_1M = _abi.MP1M_JAC_OUT
JACOBIAN_WRT_1M = _abi.MP1M_JAC_WRT


def jacobian_1m(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, wrt=JACOBIAN_WRT_1M, with_tendencies=False, *, out=None, stream=None) -> Jacobian1M:
    """The Jacobian of the 1-moment tendencies `bulk_microphysics_tendencies_1m(Instantaneous(), …)` (BMT:505-514 → :141-252) with respect to the state,
    behind `cmx_mp1m_jacobian_*`: the same point function, evaluated on forward-mode dual numbers in one kernel — the true derivatives, not the donor-based
    linearization inside LinearizedAverage (BMT:269-379).

    `wrt`: the inputs to differentiate, any subset of `JACOBIAN_WRT_1M` = ("T", "q_tot", "q_lcl", "q_icl", "q_rai", "q_sno") in any order (ρ is held
    fixed).  Returns `Jacobian1M(jac, tendencies, wrt)`: `jac` is one contiguous tensor of shape (4, len(wrt), *rho.shape) with
    `jac[o, k]` = ∂`JACOBIAN_OUTPUTS_1M[o]`/∂`wrt[k]` (its slices are the columns handed to the ABI; a column does not depend on which others are
    requested); `tendencies` is a (4, *rho.shape) tensor, bit-identical to `bulk_microphysics_tendencies_1m(Instantaneous(), …)` on the same columns,
    with `with_tendencies=True`, else None.  `out=(jac, tendencies)` lets the caller provide either tensor (None: allocated here; each slice
    `[o, k]` / `[o]` must be contiguous).  An implicit step solves (I − Δt·J) δ = Δt·f per point from these columns.
    Asynchronous on `stream` (default: torch's current stream)."""
    if not isinstance(mp, Microphysics1MParams):
        raise TypeError("mp must be Microphysics1MParams")
    return Jacobian1M(*_jacobian("cmx_mp1m_jacobian", mp, mp.flags, tps, (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), _NAMES, JACOBIAN_WRT_1M,
                                 _abi.CMX_MP1M_JAC_NOUT, wrt, with_tendencies, out, stream))


Jvp1M = namedtuple("Jvp1M", ["jvp", "tendencies"])
Vjp1M = namedtuple("Vjp1M", ["grad", "tendencies", "wrt"])


def jvp_1m(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, tangents, with_tendencies=False, *, out=None, stream=None) -> Jvp1M:
    """J v of the 1-moment tendencies (Instantaneous mode) behind `cmx_mp1m_jvp_*`: the directional derivative of the four tendencies along `tangents`
    (dict name -> tensor over `JACOBIAN_WRT_1M`; a missing name is a zero tangent, a `rho` tangent a ValueError), one evaluation of the point function on
    dual numbers.  Returns `Jvp1M(jvp, tendencies)` with `jvp` of shape (4, *rho.shape) in the order of `JACOBIAN_OUTPUTS_1M`; arguments as for
    `cmx.warm_rain_jvp_2m`."""
    if not isinstance(mp, Microphysics1MParams):
        raise TypeError("mp must be Microphysics1MParams")
    return Jvp1M(*_jvp("cmx_mp1m_jvp", mp, mp.flags, tps, (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), _NAMES, JACOBIAN_WRT_1M, _abi.CMX_MP1M_JAC_NOUT,
                       tangents, with_tendencies, out, stream))


def vjp_1m(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, cotangents, wrt=JACOBIAN_WRT_1M, with_tendencies=False, *, out=None, stream=None) -> Vjp1M:
    """Jᵀḡ of the 1-moment tendencies (Instantaneous mode) behind `cmx_mp1m_vjp_*`: `cotangents` a sequence of 4 tensors or None in the order of
    `JACOBIAN_OUTPUTS_1M` (None removes that output from the sum), `wrt` any subset of `JACOBIAN_WRT_1M`.  Returns `Vjp1M(grad, tendencies, wrt)` with
    `grad` of shape (len(wrt), *rho.shape); arguments as for `cmx.warm_rain_vjp_2m`."""
    if not isinstance(mp, Microphysics1MParams):
        raise TypeError("mp must be Microphysics1MParams")
    return Vjp1M(*_vjp("cmx_mp1m_vjp", mp, mp.flags, tps, (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), _NAMES, JACOBIAN_WRT_1M, _abi.CMX_MP1M_JAC_NOUT,
                       cotangents, wrt, with_tendencies, out, stream))


ParamJvp1M = namedtuple("ParamJvp1M", ["jvp", "tendencies"])
ParamVjp1M = namedtuple("ParamVjp1M", ["grad", "tendencies", "wrt"])


def param_jvp_1m(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, directions, with_tendencies=False, *, out=None, stream=None) -> ParamJvp1M:
    """The derivative of the 1-moment tendencies (Instantaneous mode) with respect to the scheme's PARAMETERS along `directions`, behind
    `cmx_mp1m_param_jvp_*`: jvp[d, o] = Σ_p ∂`JACOBIAN_OUTPUTS_1M[o]`/∂θ_p·δθ_p⁽ᵈ⁾ per point.  `directions`: {ClimaParams name: weight} mappings
    (`parameters.MICROPHYSICS_1M_DIRECTION_NAMES`) or (d_mp, d_thermo) pairs of `parameters.parameter_direction`.  Returns `ParamJvp1M(jvp, tendencies)`, `jvp` of
    shape (len(directions), 4, *rho.shape); `tendencies` are bit-identical to `bulk_microphysics_tendencies_1m` unless a direction moves a size-relation
    exponent of rain or snow (then the run-time-flags instantiation runs: agreement to the parity bound).  Arguments as for `cmx.warm_rain_param_jvp_2m`."""
    return ParamJvp1M(*_param_jvp("cmx_mp1m_param_jvp", mp, mp.flags, tps, (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), _NAMES, _abi.CMX_MP1M_JAC_NOUT,
                                  directions, with_tendencies, out, stream))


def param_vjp_1m(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, cotangents, wrt, with_tendencies=False, *, out=None, stream=None) -> ParamVjp1M:
    """The gradient of L = Σ_points Σ_o ḡ_o·out_o of the 1-moment tendencies with respect to the scheme's PARAMETERS, behind `cmx_mp1m_param_vjp_*`:
    grad[k] = dL/d`wrt[k]`, a deterministic reduction over the points in float64.  `wrt`: ClimaParams names or directions.  Returns
    `ParamVjp1M(grad, tendencies, wrt)`; arguments and rules as for `cmx.warm_rain_param_vjp_2m`."""
    return ParamVjp1M(*_param_vjp("cmx_mp1m_param_vjp", mp, mp.flags, tps, (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), _NAMES, _abi.CMX_MP1M_JAC_NOUT,
                                  cotangents, wrt, with_tendencies, out, stream))


Implicit1M = namedtuple("Implicit1M", ["implicit", "tendencies"])


def implicit_tendencies_1m(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, dt, with_tendencies=False, *, out=None, stream=None) -> Implicit1M:
    """The tendency of a linearly implicit (Rosenbrock–Euler) step of the 1-moment tendencies (Instantaneous mode) behind `cmx_mp1m_implicit_tendencies_*`:
    r = (I − dt·J)⁻¹ f per point with J the true Jacobian with respect to (q_lcl, q_icl, q_rai, q_sno) — the 4 × 4 block of `jacobian_1m`, not the donor-based
    linearization of LinearizedAverage — solved in registers in the pass that computes it.  Returns `Implicit1M(implicit, tendencies)` with `implicit` of
    shape (4, *rho.shape) in the order of `JACOBIAN_OUTPUTS_1M`; arguments as for `cmx.warm_rain_implicit_tendencies_2m`."""
    if not isinstance(mp, Microphysics1MParams):
        raise TypeError("mp must be Microphysics1MParams")
    return Implicit1M(*_implicit("cmx_mp1m_implicit_tendencies", mp, mp.flags, tps, (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), _NAMES,
                                 _abi.CMX_MP1M_JAC_NOUT, dt, with_tendencies, out, stream))


def implicit_average_1m(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, dt, nsub=1, nonnegative=True, *, out=None, stream=None):
    """The average tendency of (q_lcl, q_icl, q_rai, q_sno) over a time step `dt`, taken in `nsub` linearly implicit substeps inside one kernel
    (`cmx_mp1m_implicit_average_*`): the sub-stepping of LinearizedAverage — T follows the latent heating, T += (L_v/c_p·(Δq_lcl + Δq_rai) + L_s/c_p·(Δq_icl +
    Δq_sno)) per substep — on the true Jacobian of `jacobian_1m` instead of the donor-based linearization, every option set.  Returns a tensor of shape
    (4, *rho.shape) in the order of `JACOBIAN_OUTPUTS_1M`; arguments and rules as for `cmx.warm_rain_implicit_average_2m`."""
    if not isinstance(mp, Microphysics1MParams):
        raise TypeError("mp must be Microphysics1MParams")
    return _implicit_average("cmx_mp1m_implicit_average", mp, mp.flags, tps, (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), _NAMES, _abi.CMX_MP1M_JAC_NOUT, dt,
                             nsub, nonnegative, out, stream)


def bulk_microphysics_tendencies_1m_fields(mode, scheme, mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, dt=None, nsub=1, *, q_min=None, out=None,
                                           aos=False, stream=None):
    """The 1-moment tendencies — Instantaneous, or LinearizedAverage with `dt` [, `nsub`] — on the host model's own storage (SURVEY §8f-3,
    `cmx_mp1m_tendencies_fields_*` / `cmx_mp1m_linearized_average_fields_*`): every column
    a contiguous 1-D tensor or a (n_seg, seg_len) view with contiguous rows (a ClimaCore `VIJFH` field component in place); the result
    goes into `out` (4 tensors of the same shape → `Tendencies1M`) or, with `aos=True`, into the reference's own result layout — an
    (n, 4) tensor of NamedTuple rows (dq_lcl_dt, dq_icl_dt, dq_rai_dt, dq_sno_dt).  Bit-identical to `bulk_microphysics_tendencies_1m`."""
    if not isinstance(scheme, Microphysics1Moment) or not isinstance(mode, (Instantaneous, LinearizedAverage)):
        raise TypeError("mode must be Instantaneous() or LinearizedAverage() and scheme Microphysics1Moment()")
    if not isinstance(mp, Microphysics1MParams):
        raise TypeError("mp must be Microphysics1MParams")
    fam = _fam_of(rho)
    if fam is not mp.fam or not isinstance(tps, fam.thermo):
        raise TypeError("parameter float type does not match the state columns")
    name, extra = "cmx_mp1m_tendencies_fields", ()
    if isinstance(mode, LinearizedAverage):     # cmx_mp1m_linearized_average_fields_*: (q_min, Δt, nsub) after the flags
        if dt is None or not dt > 0 or int(nsub) < 1:
            raise ValueError("LinearizedAverage needs dt > 0 and nsub >= 1")
        if q_min is None:
            from .parameters import DEFAULT_PARAMETERS
            q_min = DEFAULT_PARAMETERS["specific_humidity_minimum"]
        name, extra = "cmx_mp1m_linearized_average_fields", (fam.ft(q_min), fam.ft(dt), C.c_int32(int(nsub)))
    elif dt is not None:
        raise TypeError("Instantaneous() takes no dt")
    r = _fields_call(name, mp.c, tps, mp.flags, (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno),
                     ("rho", "T", "q_tot", "q_lcl", "q_icl", "q_rai", "q_sno"), 4, 4, out, aos, stream, extra)
    return r if aos else Tendencies1M(*r)


def microphysics_source_terms_1m(mp, tps, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, *, stream=None) -> SourceTerms1M:
    """The 18 individual source terms of `_microphysics_source_terms` (BMT:141-217) over columns."""
    cols = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    ref, fam = _prep(mp, tps, cols)
    outs = [torch.empty_like(ref) for _ in range(_abi.CMX_MP1M_NSRC)]
    arr = (C.c_void_p * _abi.CMX_MP1M_NSRC)(*[o.data_ptr() for o in outs])
    _lib.call("cmx_mp1m_source_terms", fam, ref.device, C.byref(mp.c), C.byref(tps), mp.flags, ref.numel(), *[_ptr(t) for t in cols], arr,
              stream=stream)
    return SourceTerms1M(*outs)


def terminal_velocity_1m(mp, rho, q_rai=None, q_sno=None, *, chen=False, stream=None) -> TerminalVelocities1M:
    """Mass-weighted 1M fall speeds — CM1.terminal_velocity (CM1:223-270): Blk1M rain (needs q_rai), Blk1M snow
    (needs q_sno) and, with `chen=True`, Chen-2022 rain (Table B1; or `chen` = a Chen2022VelTypeRain struct with another table)."""
    if not isinstance(mp, Microphysics1MParams):
        raise TypeError("mp must be Microphysics1MParams")
    cols = [c for c in (rho, q_rai, q_sno) if c is not None]
    ref = _check_cols(cols, ("rho", "q", "q"))
    fam = _fam_of(ref)
    if fam is not mp.fam:
        raise TypeError("parameter float type does not match the state columns")
    if chen and q_rai is None:
        raise ValueError("the Chen-2022 rain velocity needs q_rai")
    mk = lambda on: torch.empty_like(ref) if on else None  # noqa: E731
    out = TerminalVelocities1M(mk(q_rai is not None), mk(q_sno is not None), mk(bool(chen)))
    ch = (Chen2022VelTypeRain(fam.sfx) if chen is True else chen) if chen else None
    if ch is not None and not isinstance(ch, fam.chen2022_rain_vel):
        raise TypeError("chen must be True or the Chen2022VelTypeRain struct of the state's float type")
    _lib.call("cmx_mp1m_terminal_velocity", fam, ref.device, C.byref(mp.c), C.byref(ch) if ch is not None else None, ref.numel(), _ptr(rho),
              _ptr(q_rai), _ptr(q_sno), *[_ptr(o) for o in out], stream=stream)
    return out


SedimentationVelocities = namedtuple("SedimentationVelocities", ["w_lcl", "w_icl", "w_rai", "w_sno"])


def sedimentation_velocities(mp, stokes, chen_rain, chen_ice, rho, q_lcl=None, q_icl=None, q_rai=None, q_sno=None, *,
                             stream=None) -> SedimentationVelocities:
    """The bulk fall speeds a host model precomputes for sedimentation (ClimaAtmos `set_sedimentation_precomputed_quantities`,
    test/gpu_clima_core_test.jl:36-45): cloud liquid (Stokes), cloud ice (Chen-2022 small ice), rain (Chen-2022 rain) and
    snow (Chen-2022 large ice) — `CMNonEq.terminal_velocity` (NonEq:250-281) and `CM1.terminal_velocity` (CM1:251-297).
    Species whose q column is None are skipped (None in the result)."""
    if not isinstance(mp, Microphysics1MParams):
        raise TypeError("mp must be Microphysics1MParams")
    qs = (q_lcl, q_icl, q_rai, q_sno)
    cols = [rho] + [q for q in qs if q is not None]
    ref = _check_cols(cols, ["rho"] + ["q"] * (len(cols) - 1))
    fam = _fam_of(ref)
    if fam is not mp.fam:
        raise TypeError("parameter float type does not match the state columns")
    outs = [torch.empty_like(ref) if q is not None else None for q in qs]
    ref_or_null = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    _lib.call("cmx_sedimentation_velocities", fam, ref.device, C.byref(mp.c), ref_or_null(stokes), ref_or_null(chen_rain), ref_or_null(chen_ice),
              ref.numel(), _ptr(rho), *[_ptr(q) for q in qs], *[_ptr(o) for o in outs], stream=stream)
    return SedimentationVelocities(*outs)


def snow_terminal_velocity(mp, chen_ice, rho, q_sno, snow_shape=None, *, stream=None):
    """The Chen-2022 snow fall speed over columns (`cmx_snow_terminal_velocity_*`): `CM1.terminal_velocity(snow, Ch2022.large_ice, ρ, q,
    snow_shape)` with `snow_shape = Oblate()` or `Prolate()` (CM1:299-324), or with `snow_shape=None` the fixed aspect ratio of the 4-argument
    method (CM1:272-297; bit-identical to `sedimentation_velocities(…).w_sno` wherever no input is NaN).  `chen_ice` = the
    Chen2022VelTypeIce struct of the state's float type.  Returns one new tensor."""
    if not isinstance(mp, Microphysics1MParams):
        raise TypeError("mp must be Microphysics1MParams")
    shape = _shape_of(snow_shape)
    ref = _check_cols([rho, q_sno], ["rho", "q_sno"])
    fam = _fam_of(ref)
    if fam is not mp.fam:
        raise TypeError("parameter float type does not match the state columns")
    if not isinstance(chen_ice, fam.chen2022_ice_vel):
        raise TypeError(f"chen_ice: expected the {fam.chen2022_ice_vel.__name__} struct of the state's float type, got {type(chen_ice).__name__}")
    w = torch.empty_like(ref)
    _lib.call("cmx_snow_terminal_velocity", fam, ref.device, C.byref(mp.c), C.byref(chen_ice),
              shape._shape if shape is not None else _abi.CMX_SNOW_SHAPE_ASPR, ref.numel(), _ptr(rho), _ptr(q_sno), _ptr(w), stream=stream)
    return w


ColumnStep1M = namedtuple("ColumnStep1M", ["dq_lcl_dt", "dq_icl_dt", "dq_rai_dt", "dq_sno_dt", "precip_rai", "precip_sno"])


def column_tendencies_sedimentation_1m(mode, scheme, mp, tps, stokes, chen_rain, chen_ice, inv_dz, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno,
                                       dt=None, nsub=1, *, q_min=None, precip=True, snow_shape=None, stream=None) -> ColumnStep1M:
    """The operational 1-moment column step in one pass (`cmx_mp1m_column_tendencies_sedimentation_*`): the 1-moment tendencies
    (Instantaneous, or LinearizedAverage with `dt` [, `nsub`]) + the four sedimentation velocities (`sedimentation_velocities`) + the host
    model's first-order upwind flux divergence of q_lcl, q_icl, q_rai, q_sno.  State tensors of shape (n_col, n_lev), level 0 lowest,
    contiguous; `inv_dz` = n_lev values 1/Δz.  Returns the four total tendencies and (precip=True) the surface rain / snow fluxes.
    `snow_shape` = Oblate() or Prolate(): the snow fall speed of `snow_terminal_velocity` with that shape (the CMX_1M_SED_SNOW_* bit)."""
    if not isinstance(scheme, Microphysics1Moment) or not isinstance(mode, (Instantaneous, LinearizedAverage)):
        raise TypeError("mode must be Instantaneous() or LinearizedAverage() and scheme Microphysics1Moment()")
    cols = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    names = ("rho", "T", "q_tot", "q_lcl", "q_icl", "q_rai", "q_sno")
    shape = _shape_of(snow_shape)
    if rho.dim() != 2:
        raise ValueError("state tensors must have shape (n_col, n_lev)")
    # validate the 2-D tensors THEMSELVES: the kernel reads and writes flat row-major (n_col, n_lev) storage, so a transposed
    # view, a column of another shape with the same number of elements or any non-contiguous tensor must be refused, not silently copied
    for c, nm in zip(cols, names):
        if c.shape != rho.shape:
            raise ValueError(f"column {nm}: shape {tuple(c.shape)} differs from rho's {tuple(rho.shape)}")
        if not c.is_contiguous():
            raise ValueError(f"column {nm} must be a contiguous (n_col, n_lev) tensor (levels contiguous within a column)")
    flat = [c.view(-1) for c in cols]
    ref, fam = _prep(mp, tps, flat)
    for obj, cls, nm in ((stokes, fam.stokes_vel, "stokes"), (chen_rain, fam.chen2022_rain_vel, "chen_rain"), (chen_ice, fam.chen2022_ice_vel, "chen_ice")):
        if not isinstance(obj, cls):
            raise TypeError(f"{nm}: expected the {cls.__name__} struct of the state's float type, got {type(obj).__name__}")
    n_col, n_lev = rho.shape
    if inv_dz.numel() != n_lev or inv_dz.dtype != ref.dtype or inv_dz.device != ref.device or not inv_dz.is_contiguous():
        raise ValueError("inv_dz: n_lev contiguous values of the state's dtype on the state's device")
    lin = isinstance(mode, LinearizedAverage)
    if lin:
        if dt is None or not dt > 0 or int(nsub) < 1:
            raise ValueError("LinearizedAverage needs dt > 0 and nsub >= 1")
        if q_min is None:
            from .parameters import DEFAULT_PARAMETERS
            q_min = DEFAULT_PARAMETERS["specific_humidity_minimum"]
    elif dt is not None:
        raise TypeError("Instantaneous() takes no dt")
    out = [torch.empty(rho.shape, dtype=ref.dtype, device=ref.device) for _ in range(4)]      # contiguous row-major, whatever rho's strides
    pr = [torch.empty(n_col, dtype=ref.dtype, device=ref.device) if precip else None for _ in range(2)]
    in_p = (C.c_void_p * 7)(*[c.data_ptr() for c in flat])
    out_p = (C.c_void_p * 4)(*[o.data_ptr() for o in out])
    _lib.call("cmx_mp1m_column_tendencies_sedimentation", fam, ref.device, C.byref(mp.c), C.byref(tps), C.byref(stokes), C.byref(chen_rain),
              C.byref(chen_ice), mp.flags | (shape._column_bit if shape else 0), q_min if lin else 0.0, dt if lin else 0.0, int(nsub) if lin else 0,
              n_col, n_lev, _ptr(inv_dz), in_p, out_p, _ptr(pr[0]), _ptr(pr[1]), stream=stream)
    return ColumnStep1M(*out, *pr)


ColumnJvp1M = namedtuple("ColumnJvp1M", ["jvp", "jvp_precip_rai", "jvp_precip_sno", "tendencies", "precip_rai", "precip_sno"])
ColumnVjp1M = namedtuple("ColumnVjp1M", ["grad", "tendencies", "precip_rai", "precip_sno", "wrt"])


def _column_products_head_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, cols):
    """The checks of `column_tendencies_sedimentation_1m` for the two products with its Jacobian: (reference column of shape (n_col, n_lev), float family,
    what the ABI arguments refer to, the ABI arguments from the parameter structs through `in`)."""
    rho = cols[0]
    if rho.dim() != 2:
        raise ValueError("state tensors must have shape (n_col, n_lev)")
    # the 2-D tensors THEMSELVES, as in column_tendencies_sedimentation_1m: the kernels read flat row-major (n_col, n_lev) storage
    for c, nm in zip(cols, _NAMES):
        if c.shape != rho.shape:
            raise ValueError(f"column {nm}: shape {tuple(c.shape)} differs from rho's {tuple(rho.shape)}")
        if not c.is_contiguous():
            raise ValueError(f"column {nm} must be a contiguous (n_col, n_lev) tensor (levels contiguous within a column)")
    _, fam = _prep(mp, tps, [c.view(-1) for c in cols])
    for obj, cls, nm in ((stokes, fam.stokes_vel, "stokes"), (chen_rain, fam.chen2022_rain_vel, "chen_rain"), (chen_ice, fam.chen2022_ice_vel, "chen_ice")):
        if not isinstance(obj, cls):
            raise TypeError(f"{nm}: expected the {cls.__name__} struct of the state's float type, got {type(obj).__name__}")
    n_col, n_lev = rho.shape
    if inv_dz.numel() != n_lev or inv_dz.dtype != rho.dtype or inv_dz.device != rho.device or not inv_dz.is_contiguous():
        raise ValueError("inv_dz: n_lev contiguous values of the state's dtype on the state's device")
    in_p = (C.c_void_p * 7)(*[c.data_ptr() for c in cols])
    return rho, fam, in_p, (C.byref(mp.c), C.byref(tps), C.byref(stokes), C.byref(chen_rain), C.byref(chen_ice), mp.flags, n_col, n_lev, _ptr(inv_dz), in_p)


def _column_primal_out_1m(ref, with_tendencies):
    if not with_tendencies:
        return None, None, None
    return (torch.empty((4, *ref.shape), dtype=ref.dtype, device=ref.device), torch.empty(ref.shape[0], dtype=ref.dtype, device=ref.device),
            torch.empty(ref.shape[0], dtype=ref.dtype, device=ref.device))


def column_jvp_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, tangents, with_tendencies=False, *,
                  stream=None) -> ColumnJvp1M:
    """J v of `column_tendencies_sedimentation_1m(Instantaneous(), …)` — the four tendencies WITH the upwind flux divergence of the four falling species —
    and of its two precipitation fluxes, behind `cmx_mp1m_column_jvp_*` (include/cmx.h §27): the matvec of a Newton–Krylov solver that treats 1-moment
    microphysics and sedimentation implicitly together.  One launch; ρ and `inv_dz` are held fixed.

    Parameters, `inv_dz` and the state columns of shape (n_col, n_lev) as for `column_tendencies_sedimentation_1m`.  `tangents`: dict name -> tensor of the
    state's shape over `JACOBIAN_WRT_1M`; a missing name is a zero tangent, a `rho` tangent a ValueError.  Returns `ColumnJvp1M(jvp, jvp_precip_rai,
    jvp_precip_sno, tendencies, precip_rai, precip_sno)`: `jvp` of shape (4, n_col, n_lev) in the order of `JACOBIAN_OUTPUTS_1M`, `jvp_precip_*` (n_col,);
    with `with_tendencies=True` also `tendencies` (4, n_col, n_lev) and `precip_*` (n_col,), bit-identical to the primal wrapper, else None.  Asynchronous on
    `stream`."""
    if not isinstance(tangents, dict):
        raise TypeError("tangents must be a dict: name of a differentiable input -> tensor")
    _check_wrt(tangents.keys(), JACOBIAN_WRT_1M, "tangents")
    cols = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    ref, fam, keep, head = _column_products_head_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, cols)
    given = [(k, v) for k, v in tangents.items() if v is not None]
    if given:
        _check_cols([ref] + [v for _, v in given], ["rho"] + [f"tangent of {k}" for k, _ in given])
    jvp = torch.empty((4, *ref.shape), dtype=ref.dtype, device=ref.device)
    jvp_precip = torch.empty((2, ref.shape[0]), dtype=ref.dtype, device=ref.device)
    tend, pr, ps = _column_primal_out_1m(ref, with_tendencies)
    _lib.call("cmx_mp1m_column_jvp", fam, ref.device, *head, _table([tangents.get(name) for name in JACOBIAN_WRT_1M]), _table([jvp[o] for o in range(4)]),
              _ptr(jvp_precip[0]), _ptr(jvp_precip[1]), _table([tend[o] for o in range(4)]) if tend is not None else None, _ptr(pr), _ptr(ps), stream=stream)
    return ColumnJvp1M(jvp, jvp_precip[0], jvp_precip[1], tend, pr, ps)


def column_vjp_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, cotangents, cot_precip_rai=None,
                  cot_precip_sno=None, wrt=JACOBIAN_WRT_1M, with_tendencies=False, *, stream=None) -> ColumnVjp1M:
    """Jᵀḡ of `column_tendencies_sedimentation_1m(Instantaneous(), …)` and its precipitation fluxes behind `cmx_mp1m_column_vjp_*` (include/cmx.h §27): the
    gradient of Σ ḡ·tendencies + Σ p̄_rai·precip_rai + Σ p̄_sno·precip_sno with respect to the inputs `wrt` — what
    `loss(precip_rai + precip_sno).backward()` needs (cmx.autograd).  One launch.

    `cotangents`: a sequence of 4 tensors of the state's shape or None in the order of `JACOBIAN_OUTPUTS_1M` (None: that output is not part of the sum), or
    None for none at all; `cot_precip_rai`, `cot_precip_sno`: tensors of n_col values or None.  `wrt`: any subset of `JACOBIAN_WRT_1M` in any order.  Returns
    `ColumnVjp1M(grad, tendencies, precip_rai, precip_sno, wrt)`: `grad` of shape (len(wrt), n_col, n_lev) — a cotangent at level k reaches the gradients at
    levels k and k + 1 of its column; a gradient does not depend on which others are requested.  The other arguments as for `column_jvp_1m`."""
    wrt = _check_wrt(wrt, JACOBIAN_WRT_1M)
    cotangents = [None] * 4 if cotangents is None else list(cotangents)
    if len(cotangents) != 4:
        raise ValueError("cotangents: 4 tensors (or None) expected, one per output")
    if not wrt and not with_tendencies:
        raise ValueError("nothing to compute: wrt is empty and with_tendencies is False")
    cols = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    ref, fam, keep, head = _column_products_head_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, cols)
    given = [(o, g) for o, g in enumerate(cotangents) if g is not None]
    if given:
        _check_cols([ref] + [g for _, g in given], ["rho"] + [f"cotangent {o}" for o, _ in given])
    for nm, p in (("cot_precip_rai", cot_precip_rai), ("cot_precip_sno", cot_precip_sno)):
        if p is not None and (p.dtype != ref.dtype or p.device != ref.device or p.shape != (ref.shape[0],) or not p.is_contiguous()):
            raise ValueError(f"{nm} must be a contiguous device vector of n_col values of the state dtype")
    grad = torch.empty((len(wrt), *ref.shape), dtype=ref.dtype, device=ref.device)
    grads = [None] * len(JACOBIAN_WRT_1M)
    for k, name in enumerate(wrt):
        grads[JACOBIAN_WRT_1M.index(name)] = grad[k]
    tend, pr, ps = _column_primal_out_1m(ref, with_tendencies)
    _lib.call("cmx_mp1m_column_vjp", fam, ref.device, *head, _table(cotangents), _ptr(cot_precip_rai), _ptr(cot_precip_sno), _table(grads),
              _table([tend[o] for o in range(4)]) if tend is not None else None, _ptr(pr), _ptr(ps), stream=stream)
    return ColumnVjp1M(grad, tend, pr, ps, wrt)


ColumnParamJvp1M = namedtuple("ColumnParamJvp1M", ["jvp", "jvp_precip_rai", "jvp_precip_sno", "tendencies", "precip_rai", "precip_sno"])
ColumnParamVjp1M = namedtuple("ColumnParamVjp1M", ["grad", "tendencies", "precip_rai", "precip_sno", "wrt"])


def _column_param_directions_1m(mp, fam, directions, stokes, chen_rain, chen_ice):
    """The five direction tables of include/cmx.h §28 from a sequence whose members are {ClimaParams name: weight} mappings or the 5-tuples of
    `parameters.column_parameter_direction_1m`."""
    quints = [column_parameter_direction_1m(mp, d, stokes, chen_rain, chen_ice) if isinstance(d, dict) else tuple(d) for d in directions]
    if not quints:
        raise ValueError("directions: at least one direction expected")
    types = (fam.microphysics_1m, fam.thermo, fam.stokes_vel, fam.chen2022_rain_vel, fam.chen2022_ice_vel)
    for q in quints:
        if len(q) != 5 or not all(isinstance(a, t) for a, t in zip(q, types)):
            raise TypeError("directions: (d_microphysics_1m, d_thermo, d_stokes_vel, d_chen2022_rain_vel, d_chen2022_ice_vel) structs of the state's float "
                            "type, or {name: weight} mappings")
    return [(t * len(quints))(*[q[k] for q in quints]) for k, t in enumerate(types)]


def column_param_jvp_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, directions, with_tendencies=False, *,
                        stream=None) -> ColumnParamJvp1M:
    """J_θ·δθ of `column_tendencies_sedimentation_1m(Instantaneous(), …)` — the four tendencies with the flux divergence of the four falling species — and of
    its two precipitation fluxes with respect to the scheme's PARAMETERS, the fall-speed parameters included, behind `cmx_mp1m_column_param_jvp_*`
    (include/cmx.h §28).  The state, ρ and `inv_dz` are held fixed.

    Arguments as for `column_jvp_1m`; `directions`: a sequence of {ClimaParams name: weight} mappings (`parameters.COLUMN_1M_DIRECTION_NAMES` has the names)
    or of the 5-tuples of `parameters.column_parameter_direction_1m`.  Returns `ColumnParamJvp1M(jvp, jvp_precip_rai, jvp_precip_sno, tendencies, precip_rai,
    precip_sno)`: `jvp` of shape (len(directions), 4, n_col, n_lev), `jvp_precip_*` (len(directions), n_col); a column does not depend on which other
    directions are in the call.  More than `CMX_PARAM_MAX_DIRS` = 16 directions are several calls.  b and b_ρ of the Chen-2022 rain table are held fixed: a
    direction on them raises CmxStatusError (CMX_ERR_UNSUPPORTED).  Asynchronous on `stream`."""
    cols = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    ref, fam, keep, head = _column_products_head_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, cols)
    tables = _column_param_directions_1m(mp, fam, directions, stokes, chen_rain, chen_ice)
    ndir = len(tables[0])
    jvp = torch.empty((ndir, 4, *ref.shape), dtype=ref.dtype, device=ref.device)
    jvp_precip = torch.empty((2, ndir, ref.shape[0]), dtype=ref.dtype, device=ref.device)
    tend, pr, ps = _column_primal_out_1m(ref, with_tendencies)
    for d0 in range(0, ndir, _abi.CMX_PARAM_MAX_DIRS):
        nd = min(_abi.CMX_PARAM_MAX_DIRS, ndir - d0)
        first = d0 == 0 and tend is not None
        _lib.call("cmx_mp1m_column_param_jvp", fam, ref.device, *head, nd, *[C.byref(t[d0]) for t in tables],
                  _table([jvp[d, o] for d in range(d0, d0 + nd) for o in range(4)]), _table([jvp_precip[0, d] for d in range(d0, d0 + nd)]),
                  _table([jvp_precip[1, d] for d in range(d0, d0 + nd)]), _table([tend[o] for o in range(4)]) if first else None,
                  _ptr(pr) if first else None, _ptr(ps) if first else None, stream=stream)
    return ColumnParamJvp1M(jvp, jvp_precip[0], jvp_precip[1], tend, pr, ps)


def column_param_vjp_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, cotangents, cot_precip_rai=None,
                        cot_precip_sno=None, wrt=(), with_tendencies=False, *, stream=None) -> ColumnParamVjp1M:
    """The gradient of Σ ḡ·tendencies + Σ p̄_rai·precip_rai + Σ p̄_sno·precip_sno of `column_tendencies_sedimentation_1m(Instantaneous(), …)` with respect to
    the PARAMETERS behind `cmx_mp1m_column_param_vjp_*` (include/cmx.h §28): what `loss(precip_rai + precip_sno).backward()` needs to reach `theta`
    (cmx.autograd).

    `cotangents`, `cot_precip_rai`, `cot_precip_sno` as for `column_vjp_1m`; `wrt`: ClimaParams names (one-hot directions) or directions as for
    `column_param_jvp_1m`.  Returns `ColumnParamVjp1M(grad, tendencies, precip_rai, precip_sno, wrt)`: `grad` a float64 tensor of len(wrt) values on the
    state's device — a fixed-order reduction, bit-identical from run to run."""
    wrt = tuple(wrt)
    cotangents = [None] * 4 if cotangents is None else list(cotangents)
    if len(cotangents) != 4:
        raise ValueError("cotangents: 4 tensors (or None) expected, one per output")
    cols = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
    ref, fam, keep, head = _column_products_head_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, cols)
    tables = _column_param_directions_1m(mp, fam, [{w: 1.0} if isinstance(w, str) else w for w in wrt], stokes, chen_rain, chen_ice)
    given = [(o, g) for o, g in enumerate(cotangents) if g is not None]
    if given:
        _check_cols([ref] + [g for _, g in given], ["rho"] + [f"cotangent {o}" for o, _ in given])
    for nm, p in (("cot_precip_rai", cot_precip_rai), ("cot_precip_sno", cot_precip_sno)):
        if p is not None and (p.dtype != ref.dtype or p.device != ref.device or p.shape != (ref.shape[0],) or not p.is_contiguous()):
            raise ValueError(f"{nm} must be a contiguous device vector of n_col values of the state dtype")
    ndir = len(tables[0])
    grad = torch.empty(ndir, dtype=torch.float64, device=ref.device)
    workspace = torch.empty(min(ndir, _abi.CMX_PARAM_MAX_DIRS) * _abi.CMX_PARAM_VJP_PARTIALS, dtype=torch.float64, device=ref.device)
    tend, pr, ps = _column_primal_out_1m(ref, with_tendencies)
    for d0 in range(0, ndir, _abi.CMX_PARAM_MAX_DIRS):
        nd = min(_abi.CMX_PARAM_MAX_DIRS, ndir - d0)
        first = d0 == 0 and tend is not None
        _lib.call("cmx_mp1m_column_param_vjp", fam, ref.device, *head, _table(cotangents), _ptr(cot_precip_rai), _ptr(cot_precip_sno), nd,
                  *[C.byref(t[d0]) for t in tables], _ptr(grad[d0:]), _ptr(workspace), _table([tend[o] for o in range(4)]) if first else None,
                  _ptr(pr) if first else None, _ptr(ps) if first else None, stream=stream)
    return ColumnParamVjp1M(grad, tend, pr, ps, wrt)


def _column_implicit_1m(entry, mp, tps, stokes, chen_rain, chen_ice, inv_dz, cols, dt, nsub, nonnegative, precip, stream):
    """The checks and the call of the two 1-moment column steps that take the implicit average as tendency (include/cmx.h §(20), §(21)): same arguments."""
    dt, nsub = _check_step(dt, nsub)
    rho = cols[0]
    if rho.dim() != 2:
        raise ValueError("state tensors must have shape (n_col, n_lev)")
    # the 2-D tensors THEMSELVES, as in column_tendencies_sedimentation_1m: the kernel reads flat row-major (n_col, n_lev) storage
    for c, nm in zip(cols, _NAMES):
        if c.shape != rho.shape:
            raise ValueError(f"column {nm}: shape {tuple(c.shape)} differs from rho's {tuple(rho.shape)}")
        if not c.is_contiguous():
            raise ValueError(f"column {nm} must be a contiguous (n_col, n_lev) tensor (levels contiguous within a column)")
    flat = [c.view(-1) for c in cols]
    ref, fam = _prep(mp, tps, flat)
    _check_step_normal(dt, nsub, ref.dtype)
    for obj, cls, nm in ((stokes, fam.stokes_vel, "stokes"), (chen_rain, fam.chen2022_rain_vel, "chen_rain"), (chen_ice, fam.chen2022_ice_vel, "chen_ice")):
        if not isinstance(obj, cls):
            raise TypeError(f"{nm}: expected the {cls.__name__} struct of the state's float type, got {type(obj).__name__}")
    n_col, n_lev = rho.shape
    if inv_dz.numel() != n_lev or inv_dz.dtype != ref.dtype or inv_dz.device != ref.device or not inv_dz.is_contiguous():
        raise ValueError("inv_dz: n_lev contiguous values of the state's dtype on the state's device")
    out = [torch.empty(rho.shape, dtype=ref.dtype, device=ref.device) for _ in range(4)]
    pr = [torch.empty(n_col, dtype=ref.dtype, device=ref.device) if precip else None for _ in range(2)]
    in_p = (C.c_void_p * 7)(*[c.data_ptr() for c in flat])
    out_p = (C.c_void_p * 4)(*[o.data_ptr() for o in out])
    _lib.call(entry, fam, ref.device, C.byref(mp.c), C.byref(tps), C.byref(stokes), C.byref(chen_rain),
              C.byref(chen_ice), mp.flags, dt, nsub, _abi.CMX_STEP_NONNEGATIVE if nonnegative else 0, n_col, n_lev, _ptr(inv_dz), in_p, out_p,
              _ptr(pr[0]), _ptr(pr[1]), stream=stream)
    return ColumnStep1M(*out, *pr)


def column_implicit_average_sedimentation_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, dt, nsub=1,
                                             nonnegative=True, *, precip=True, stream=None) -> ColumnStep1M:
    """The 1-moment column step with the sub-stepped implicit average as tendency operator (`cmx_mp1m_column_implicit_average_sedimentation_*`): per point
    the average tendency of `implicit_average_1m(…, dt, nsub, nonnegative)` — bit for bit, built on the true Jacobian where LinearizedAverage carries a
    donor-based approximation — plus, in the same kernel, the four sedimentation fluxes and the first-order upwind flux divergence of
    `column_tendencies_sedimentation_1m`, with the fluxes of the INITIAL state (sedimentation stays explicit).  include/cmx.h §(20) has the definition.

    State tensors of shape (n_col, n_lev), level 0 lowest, contiguous (a transposed view is refused, not copied); `inv_dz` = n_lev values 1/Δz; `dt`, `nsub`,
    `nonnegative` as for `implicit_average_1m`.  Returns the four total tendencies and (precip=True) the surface rain / snow fluxes.  No snow shape, no
    autograd.  Asynchronous on `stream` (default: torch's current stream)."""
    return _column_implicit_1m("cmx_mp1m_column_implicit_average_sedimentation", mp, tps, stokes, chen_rain, chen_ice, inv_dz,
                               (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), dt, nsub, nonnegative, precip, stream)


def column_implicit_step_1m(mp, tps, stokes, chen_rain, chen_ice, inv_dz, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, dt, nsub=1, nonnegative=True, *,
                            precip=True, stream=None) -> ColumnStep1M:
    """The 1-moment column step that is stable and positive at any Courant number Δt·w/Δz (`cmx_mp1m_column_implicit_step_*`): the average tendency of
    `implicit_average_1m(…, dt, nsub, nonnegative)` per point — bit for bit — and, in the same kernel, BACKWARD-EULER first-order upwind sedimentation of
    the four species, a top-down recurrence along each column with the fall speeds of the initial state.  Where
    `column_implicit_average_sedimentation_1m` (explicit fluxes) needs Δt·w/Δz ≤ 1, this step needs no sub-cycling.  The surface fluxes are those that leave
    the column DURING the step (G_0, not the initial F_0): the column budget closes.  include/cmx.h §(21) has the definition.

    Arguments, result and checks are those of `column_implicit_average_sedimentation_1m`.  No snow shape, no autograd.  Asynchronous on `stream`."""
    return _column_implicit_1m("cmx_mp1m_column_implicit_step", mp, tps, stokes, chen_rain, chen_ice, inv_dz, (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), dt,
                               nsub, nonnegative, precip, stream)
