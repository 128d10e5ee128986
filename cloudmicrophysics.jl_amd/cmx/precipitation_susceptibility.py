"""SB2006 precipitation susceptibilities over columns — host-side mirror of `CloudMicrophysics.PrecipitationSusceptibility`
(src/PrecipitationSusceptibility.jl), evaluated by the gfx950 kernel of include/cmx.h §(12).

Reference calls being replaced, point by point through ForwardDiff (:36-79):

    CMPS.precipitation_susceptibility_autoconversion(sb2006, q_lcl, q_rai, ρ, N_lcl)
    CMPS.precipitation_susceptibility_accretion(sb2006, q_lcl, q_rai, ρ, N_lcl)

Each returns the logarithmic derivatives of the rain source with respect to ln q_lcl, ln q_rai, ln N_lcl (and a zero for ln N_rai).  The device
evaluates their closed forms; the formulas and the NaN contract (a process whose rate the reference gates to zero has NaN susceptibilities) are in
include/cmx.h.  Specific contents in kg/kg, ρ in kg/m³, N_lcl per m³.  `scheme` is what `parameters.SB2006(FT)` returns.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _lib
from ._cols import _check_cols, _fam_of, _ptr

# the reference's struct (:16-21), field for field
precip_susceptibility_rates = namedtuple("precip_susceptibility_rates",
                                         ["d_ln_pp_d_ln_q_lcl", "d_ln_pp_d_ln_q_rai", "d_ln_pp_d_ln_N_lcl", "d_ln_pp_d_ln_N_rai"])
PrecipitationSusceptibilities = namedtuple("PrecipitationSusceptibilities", ["autoconversion", "accretion"])

_NAMES = ("q_lcl", "q_rai", "rho", "N_lcl")


def _run(scheme, cols, acnv, accr, stream):
    ref = _check_cols(list(cols), _NAMES)
    fam = _fam_of(ref)
    if not isinstance(scheme, fam.sb2006):
        raise TypeError("scheme must be the parameters.SB2006 of the columns' float type")
    new = lambda on: [torch.empty_like(ref) if on else None for _ in range(3)]  # noqa: E731
    au, ac = new(acnv), new(accr)
    _lib.call("cmx_sb2006_precip_susceptibility", fam, ref.device, C.byref(scheme.acnv) if acnv else None, C.byref(scheme.accr) if accr else None,
              ref.numel(), *[_ptr(c) for c in cols], *[_ptr(o) for o in au + ac], stream=stream)
    # d_ln_pp_d_ln_N_rai = zero(q_lcl) in the reference: one stored zero seen as a column (no kernel writes it, no memory traffic)
    zero = torch.zeros((), dtype=ref.dtype, device=ref.device).expand(ref.shape)
    return (precip_susceptibility_rates(*au, zero) if acnv else None), (precip_susceptibility_rates(*ac, zero) if accr else None)


def precipitation_susceptibility_autoconversion(scheme, q_lcl, q_rai, rho, N_lcl, *, stream=None) -> precip_susceptibility_rates:
    """PrecipitationSusceptibility.precipitation_susceptibility_autoconversion (:36-51) over columns."""
    return _run(scheme, (q_lcl, q_rai, rho, N_lcl), True, False, stream)[0]


def precipitation_susceptibility_accretion(scheme, q_lcl, q_rai, rho, N_lcl, *, stream=None) -> precip_susceptibility_rates:
    """PrecipitationSusceptibility.precipitation_susceptibility_accretion (:66-79) over columns."""
    return _run(scheme, (q_lcl, q_rai, rho, N_lcl), False, True, stream)[1]


def precipitation_susceptibilities(scheme, q_lcl, q_rai, rho, N_lcl, *, stream=None) -> PrecipitationSusceptibilities:
    """Both processes in one pass over the four columns: (autoconversion, accretion), each a `precip_susceptibility_rates`."""
    return PrecipitationSusceptibilities(*_run(scheme, (q_lcl, q_rai, rho, N_lcl), True, True, stream))
