"""The adiabatic parcel model over an ensemble of parcels — host-side mirror of the reference's parcel/ParcelModel.jl (with ParcelTendencies.jl,
ParcelDistributions.jl, ParcelCommon.jl), evaluated by the two gfx950 kernels of include/cmx.h §(13): one parcel per lane, the time loop inside the
kernel.

Reference calls being replaced, one parcel and one ODE solve at a time:

    pp = parcel_params{FT}(; deposition = "ABDINM", condensation_growth = "Condensation", …)
    sol = run_parcel(IC, t_0, t_end, pp)            # ODE.Euler(), dt = const_dt      ParcelModel.jl:230-366
    parcel_model(dY, Y, p, t)                        # the right-hand side             :54-187

Here `IC` is the reference's ten rows [Sₗ, p_air, T, qᵥ, qₗ, qᵢ, Nₐ, Nₗ, Nᵢ, ln(INPC)], each a scalar or a CUDA tensor of n parcels, `w` a scalar
or a tensor, and `coefficients` optionally overrides, per parcel, the coefficient pair of the activity-based schemes (calibration ensembles):
deposition_m, deposition_c, ABIFM_m, ABIFM_c, linear_c1, linear_c2.  Row 10 (ln INPC) only matters to the stochastic Frostenberg option, which is
not built; it is returned unchanged.  Options the library does not build raise NotImplementedError naming the option; strings the reference does
not know raise ValueError with the reference's message.  SI units throughout; number concentrations per kg of air as in the reference's examples.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple
from typing import Mapping, Optional

import torch

from . import _abi, _lib
from . import parameters as P

STATE = _abi.PARCEL_STATE_COLUMNS
PROCESS = _abi.PARCEL_PROCESS_COLUMNS
COEFFICIENTS = _abi.PARCEL_COEFFICIENT_COLUMNS
MAX_STEPS_PER_LAUNCH = _abi.CMX_PARCEL_MAX_STEPS_PER_LAUNCH

# option string → (flag bits | None where the library does not build it); the messages are the reference's `throw`s (ParcelModel.jl:233-333)
_OPTIONS = {
    "aerosol_act": ("Unrecognized aerosol activation mode", {"None": 0, "AeroAct": _abi.CMX_PARCEL_AERO_ACT}),
    "deposition": ("Unrecognized deposition mode", {
        "None": 0, "MohlerAF": _abi.CMX_PARCEL_DEP_MOHLER_AF, "MohlerRate": None, "ABDINM": _abi.CMX_PARCEL_DEP_ABDINM,
        "P3_dep": _abi.CMX_PARCEL_DEP_P3}),
    "heterogeneous": ("Unrecognized heterogeneous mode", {
        "None": 0, "ABIFM": _abi.CMX_PARCEL_HET_ABIFM, "P3_het": _abi.CMX_PARCEL_HET_P3, "Frostenberg_random": None,
        "Frostenberg_mean": _abi.CMX_PARCEL_HET_FROSTENBERG_MEAN, "Frostenberg_stochastic": None}),
    "homogeneous": ("Unrecognized homogeneous mode", {"None": 0, "ABHOM": _abi.CMX_PARCEL_HOM_ABHOM, "P3_hom": _abi.CMX_PARCEL_HOM_P3}),
    "condensation_growth": ("Unrecognized condensation growth mode", {
        "None": 0, "Condensation": _abi.CMX_PARCEL_COND_CONDENSATION, "NonEq_Condensation_simple": _abi.CMX_PARCEL_COND_NONEQ_SIMPLE,
        "NonEq_Condensation": None}),
    "deposition_growth": ("Unrecognized deposition growth mode", {
        "None": 0, "Deposition": _abi.CMX_PARCEL_DEPGROWTH_DEPOSITION, "NonEq_Deposition_simple": _abi.CMX_PARCEL_DEPGROWTH_NONEQ_SIMPLE,
        "NonEq_Deposition": None}),
    "liq_size_distribution": ("Unrecognized size distribution", {"Monodisperse": 0, "Gamma": _abi.CMX_PARCEL_LIQ_GAMMA, "MonodisperseMix": None}),
    "ice_size_distribution": ("Unrecognized size distribution", {"Monodisperse": 0, "Gamma": _abi.CMX_PARCEL_ICE_GAMMA}),
}


class Aerosol:
    """The `aerosol` member of parcel_params as the parcel model reads it: the ABIFM, deposition_J and Mohler-2006 coefficient structs of the
    aerosol type (parameters.Illite, DepositionDust, DesertDust, …; None where the type has none: that scheme's rate is then zero, as
    `CMI_het.ABIFM_J(::AerosolType, Δa_w) = 0` in the reference) and, for AeroAct, its molar mass M and hygroscopicity κ."""

    def __init__(self, abifm=None, deposition=None, mohler=None, M: float = 0.0, kappa: float = 0.0):
        self.abifm, self.deposition, self.mohler, self.M, self.kappa = abifm, deposition, mohler, M, kappa


def _as_aerosol(fam, a) -> Aerosol:
    if a is None or isinstance(a, Aerosol):
        return a or Aerosol()
    if isinstance(a, fam.abifm_dust):
        return Aerosol(abifm=a)
    if isinstance(a, fam.deposition_dust):
        return Aerosol(deposition=a)
    if isinstance(a, fam.mohler_dust):
        return Aerosol(mohler=a)
    if hasattr(a, "kappa") and hasattr(a, "M"):            # parameters.Sulfate / Seasalt
        return Aerosol(M=a.M, kappa=a.kappa)
    raise TypeError(f"aerosol: expected parcel.Aerosol or a coefficient struct of the float type, got {type(a).__name__}")


class parcel_params:
    """parcel_params{FT}(; …) — ParcelModel.jl:12-43 — with the reference's keyword names and defaults.  `FT` is "f32" / "f64" (or a dtype).
    `.c` is the cmx_parcel_params_* struct, `.flags` the option word; `.w` the default updraft speed."""

    def __init__(self, FT, *, prescribed_thermodynamics=False, aerosol_act="None", deposition="None", heterogeneous="None", homogeneous="None",
                 condensation_growth="None", deposition_growth="None", liq_size_distribution="Monodisperse", ice_size_distribution="Monodisperse",
                 aerosol=None, aero_σ_g=0.0, wps=None, aps=None, tps=None, aap=None, ips=None, liquid=None, ice=None, const_dt=1, w=1.0,
                 r_nuc=0.5 * 1.e-4 * 1e-6, A_aer=1e-9, ip=None, Nₐ=1e8, τ_relax_liquid=None, τ_relax_ice=None, grav=None):
        td = P._td(FT)
        fam = self.fam = td.fam
        self.options = dict(aerosol_act=aerosol_act, deposition=deposition, heterogeneous=heterogeneous, homogeneous=homogeneous,
                            condensation_growth=condensation_growth, deposition_growth=deposition_growth,
                            liq_size_distribution=liq_size_distribution, ice_size_distribution=ice_size_distribution)
        self.prescribed_thermodynamics = bool(prescribed_thermodynamics)
        flags = 0
        for name, value in self.options.items():
            message, table = _OPTIONS[name]
            if value not in table:
                raise ValueError(message)
            if table[value] is None:
                raise NotImplementedError(f"parcel_params: {name} = {value!r} is not built (include/cmx.h §13 lists what is left out and why)")
            flags |= table[value]
        if self.prescribed_thermodynamics:
            raise NotImplementedError("parcel_params: prescribed_thermodynamics = true (AIDA chamber profiles) is not built")
        self.flags = flags
        self.w = float(w)
        wps = wps or P.WaterProperties(td)
        ips = ips or {}
        aer = _as_aerosol(fam, aerosol)
        c = self.c = fam.parcel_params()
        c.tps = tps or P.ThermodynamicsParameters(td)
        c.aps = aps or P.AirProperties(td)
        c.aap = aap or P.AerosolActivationParameters(td)
        c.homogeneous = ips.get("homogeneous") or P.Koop2000(td)
        c.deposition = ips.get("deposition") or P.Mohler2006(td)
        c.p3 = ips.get("p3") or P.MorrisonMilbrandt2014(td)
        c.ip = ip or P.Frostenberg2023(td)
        # an aerosol type without the coefficients of a scheme: J = 10^(0·Δa_w − ∞) = 0
        c.aerosol_abifm = aer.abifm if aer.abifm is not None else fam.abifm_dust(0.0, -math.inf)
        c.aerosol_deposition = aer.deposition if aer.deposition is not None else fam.deposition_dust(0.0, -math.inf)
        if aer.mohler is not None:
            c.aerosol_mohler = aer.mohler
        elif deposition == "MohlerAF":
            raise TypeError("deposition = 'MohlerAF' needs an aerosol with Mohler-2006 coefficients (parameters.DesertDust / ArizonaTestDust)")
        c.const_dt, c.r_nuc, c.A_aer, c.aero_sigma_g, c.aero_N = const_dt, r_nuc, A_aer, aero_σ_g, Nₐ
        c.aero_M, c.aero_kappa = aer.M, aer.kappa
        c.grav = td["gravitational_acceleration"] if grav is None else grav
        c.rho_w, c.rho_i = wps.rho_w, wps.rho_i
        # MNE.τ_relax(liquid) / (ice) of the NonEq _simple options: the relaxation timescales of the cloud condensate
        c.tau_relax_liq = td["condensation_evaporation_timescale"] if τ_relax_liquid is None else τ_relax_liquid
        c.tau_relax_ice = td["sublimation_deposition_timescale"] if τ_relax_ice is None else τ_relax_ice
        if not c.const_dt > 0:
            raise ValueError("const_dt must be positive")


ParcelTendencies = namedtuple("ParcelTendencies", ["dY", "process_rates"])
ParcelSolution = namedtuple("ParcelSolution", ["u", "trajectory", "t", "n_steps"])
ParcelSolution.__doc__ = """run_parcel's result: `u` = the final state, [10, n]; `trajectory` = [record, 10, n] or None; `t` = the record times."""


def _columns(values, names, fam=None, like=None):
    """Scalars / tensors → contiguous 1-D CUDA tensors of one dtype, device and length (scalars are expanded)."""
    tensors = [v for v in values if isinstance(v, torch.Tensor)]
    ref = like if like is not None else (tensors[0] if tensors else None)
    if ref is None:
        raise TypeError("at least one of the parcel's rows must be a CUDA tensor: the float type, device and ensemble size come from it")
    if not ref.is_cuda:
        raise ValueError("parcel states must be resident on the GPU (torch device 'cuda'); cmx has no CPU path")
    n = max([t.numel() for t in tensors] + [ref.numel()])
    out = []
    for v, nm in zip(values, names):
        if isinstance(v, torch.Tensor):
            if not v.is_cuda:
                raise ValueError(f"{nm}: parcel states must be resident on the GPU (torch device 'cuda'); cmx has no CPU path")
            if v.dtype != ref.dtype or v.device != ref.device:
                raise ValueError(f"{nm}: dtype/device differ from the other rows")
            v = v.reshape(-1)
            if v.numel() == 1 and n > 1:
                v = v.expand(n)
            if v.numel() != n:
                raise ValueError(f"{nm}: {v.numel()} parcels, the other rows have {n}")
            out.append(v.contiguous())
        else:
            out.append(torch.full((n,), float(v), dtype=ref.dtype, device=ref.device))
    return out, ref, n


def _inputs(pp, rows, w, coefficients):
    w = pp.w if w is None else w
    cols, ref, n = _columns(list(rows[:9]) + [w], STATE + ("w",))
    fam = _abi.F32 if ref.dtype == torch.float32 else _abi.F64 if ref.dtype == torch.float64 else None
    if fam is None or fam is not pp.fam:
        raise TypeError(f"the parcel rows are {ref.dtype}; parcel_params was built for {pp.fam.sfx}")
    coef = [None] * len(COEFFICIENTS)
    for name, v in (coefficients or {}).items():
        if name not in COEFFICIENTS:
            raise KeyError(f"coefficients: {name!r} is not one of {COEFFICIENTS}")
        coef[COEFFICIENTS.index(name)] = _columns([v], (name,), like=cols[0])[0][0]
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    return cols, coef, ref, n, fam, ptrs


def parcel_tendencies(Y, pp: parcel_params, *, w=None, coefficients: Optional[Mapping] = None, process_rates: bool = True, stream=None) -> ParcelTendencies:
    """parcel_model(dY, Y, p, t) over an ensemble: `Y` = the nine (or ten) rows.  Returns (dY [10, n] with a zero ln_INPC row,
    process_rates {name: tensor} — the per-process terms dN_liq_act, dN_ice_dep, dN_ice_imm, dN_ice_hom, dq_liq_ce, dq_ice_ds)."""
    cols, coef, ref, n, fam, ptrs = _inputs(pp, Y, w, coefficients)
    dY = torch.zeros((10, n), dtype=ref.dtype, device=ref.device)
    proc = torch.empty((len(PROCESS), n), dtype=ref.dtype, device=ref.device) if process_rates else None
    _lib.call("cmx_parcel_tendencies", fam, ref.device, C.byref(pp.c), pp.flags, n, ptrs(cols[:9]), C.c_void_p(cols[9].data_ptr()), ptrs(coef),
              ptrs([dY[j] for j in range(9)]), ptrs([proc[j] for j in range(len(PROCESS))]) if process_rates else None, stream=stream)
    return ParcelTendencies(dY, dict(zip(PROCESS, proc)) if process_rates else None)


def run_parcel(IC, t_0, t_end, pp: parcel_params, *, w=None, coefficients: Optional[Mapping] = None, save_every: int = 0, out=None,
               stream=None) -> ParcelSolution:
    """run_parcel(IC, t_0, t_end, pp) over an ensemble: (t_end − t_0)/const_dt forward-Euler steps in one launch sequence.  `save_every` = k > 0 also
    returns the trajectory, one record per k steps (record 0 = IC).  `out` = a [10, n] tensor to write the final state into (it may hold IC)."""
    dt = float(pp.c.const_dt)
    steps = (float(t_end) - float(t_0)) / dt
    n_steps = int(round(steps))
    if n_steps < 0 or abs(steps - n_steps) > 1e-9 * max(1.0, abs(steps)):
        raise ValueError(f"(t_end − t_0)/const_dt = {steps} is not a whole number of steps")
    if save_every < 0:
        raise ValueError("save_every must be ≥ 0")
    rows = list(IC)
    if len(rows) not in (9, 10):
        raise ValueError("IC: the reference's ten rows [Sₗ, p_air, T, qᵥ, qₗ, qᵢ, Nₐ, Nₗ, Nᵢ, ln(INPC)] (the last may be omitted)")
    cols, coef, ref, n, fam, ptrs = _inputs(pp, rows, w, coefficients)
    if out is None:
        out = torch.empty((10, n), dtype=ref.dtype, device=ref.device)
    elif out.shape != (10, n) or out.dtype != ref.dtype or out.device != ref.device or not out.is_contiguous():
        raise ValueError("out: a contiguous [10, n] tensor of the rows' dtype and device")
    ln_inpc = _columns([rows[9] if len(rows) == 10 else 0.0], ("ln_INPC",), like=cols[0])[0][0]
    n_rec = 1 + n_steps // save_every if save_every else 0
    traj9 = torch.empty((n_rec, 9, n), dtype=ref.dtype, device=ref.device) if save_every else None
    _lib.call("cmx_parcel_run", fam, ref.device, C.byref(pp.c), pp.flags, n, n_steps, save_every, ptrs(cols[:9]), C.c_void_p(cols[9].data_ptr()),
              ptrs(coef), ptrs([out[j] for j in range(9)]), C.c_void_p(traj9.data_ptr()) if save_every else None, stream=stream)
    out[9].copy_(ln_inpc)
    traj = t = None
    if save_every:
        traj = torch.cat([traj9, ln_inpc.expand(n_rec, 1, n)], dim=1)
        t = float(t_0) + dt * save_every * torch.arange(n_rec, dtype=torch.float64)
    return ParcelSolution(out, traj, t, n_steps)
