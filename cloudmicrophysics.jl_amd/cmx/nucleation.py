"""Aerosol nucleation rates over columns — host-side mirror of `CloudMicrophysics.Nucleation` (src/Nucleation.jl), the CLOUD-chamber
new-particle-formation parameterisations, evaluated by the gfx950 kernels of include/cmx.h §(11).

Reference broadcasts being replaced (KA kernels test/gpu_tests.jl:246-285, testset "Modal nucleation kernels" :1094-1153):

    output = sum(MN.h2so4_nucleation_rate(h2so4, nh3, negative_ion, T, h2so4_nuc))                       # binary + ternary
    output = MN.organic_nucleation_rate(negative_ion, monoterpene, O3, OH, T, condensation_sink, org_nuc)
    output = MN.organic_and_h2so4_nucleation_rate(h2so4, monoterpene, OH, T, condensation_sink, mix_nuc)
    output = MN.apparent_nucleation_rate(output_diam, nucleation_rate, condensation_growth_rate, coag_sink, coag_sink_input_diam, input_diam)

Concentrations per m³, T in K, condensation sink in 1/s, rates per m³ per s.  `nucleation_rates` evaluates any subset of the first three in one
pass over the columns; the per-function mirrors below call it with one output.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _lib
from ._cols import _check_cols, _fam_of, _ptr

NucleationRates = namedtuple("NucleationRates", ["binary", "ternary", "organic", "mixed"])
PrescribedNucleationRates = namedtuple("PrescribedNucleationRates", ["organic", "mixed"])


def _cols(cols, names):
    present = [(c, n) for c, n in zip(cols, names) if c is not None]
    ref = _check_cols([c for c, _ in present], [n for _, n in present])
    return ref, _fam_of(ref)


def _need(obj, typ, what):
    if not isinstance(obj, typ):
        raise TypeError(f"{what} must be the {typ.__name__} of the columns' float type")
    return C.byref(obj)


def nucleation_rates(h2so4_params=None, organic_params=None, mixed_params=None, *, h2so4=None, nh3=None, negative_ion=None, monoterpene=None, O3=None,
                     OH=None, temp=None, condensation_sink=None, want=("binary", "ternary", "organic", "mixed"), stream=None) -> NucleationRates:
    """The fused pass (`cmx_aerosol_nucleation_rates_*`): the fields of `want` among binary / ternary (h2so4_nucleation_rate, Nucleation.jl:51-90;
    binary + ternary is the reference kernel's sum), organic (organic_nucleation_rate, :106-135) and mixed (organic_and_h2so4_nucleation_rate,
    :172-190); the others are None.  Only the columns and parameter structs the requested outputs read are needed."""
    want = tuple(want)
    unknown = set(want) - set(NucleationRates._fields)
    if unknown or not want:
        raise ValueError(f"want must name some of {NucleationRates._fields}, got {want!r}")
    names = ("h2so4", "nh3", "negative_ion", "monoterpene", "O3", "OH", "temp", "condensation_sink")
    cols = (h2so4, nh3, negative_ion, monoterpene, O3, OH, temp, condensation_sink)
    ref, fam = _cols(cols, names)
    need = set()
    if {"binary", "ternary"} & set(want):
        need |= {"h2so4", "nh3", "negative_ion", "temp"}
    if "organic" in want:
        need |= {"negative_ion", "monoterpene", "O3", "OH", "temp", "condensation_sink"}
    if "mixed" in want:
        need |= {"h2so4", "monoterpene", "OH", "temp", "condensation_sink"}
    missing = [n for n, c in zip(names, cols) if n in need and c is None]
    if missing:
        raise ValueError(f"column(s) {missing} needed for {want}")
    hp = _need(h2so4_params, fam.h2so4_nucleation, "h2so4_params") if {"binary", "ternary"} & set(want) else None
    op = _need(organic_params, fam.organic_nucleation, "organic_params") if "organic" in want else None
    mp = _need(mixed_params, fam.mixed_nucleation, "mixed_params") if "mixed" in want else None
    outs = {k: (torch.empty_like(ref) if k in want else None) for k in NucleationRates._fields}
    _lib.call("cmx_aerosol_nucleation_rates", fam, ref.device, hp, op, mp, ref.numel(),
              *[_ptr(c if n in need else None) for n, c in zip(names, cols)], *[_ptr(outs[k]) for k in NucleationRates._fields], stream=stream)
    return NucleationRates(*[outs[k] for k in NucleationRates._fields])


def h2so4_nucleation_rate(h2so4_conc, nh3_conc, negative_ion_conc, temp, params, *, stream=None):
    """Nucleation.h2so4_nucleation_rate (Nucleation.jl:51-90) → (binary_rate, ternary_rate), Dunne et al. (2016)."""
    r = nucleation_rates(params, h2so4=h2so4_conc, nh3=nh3_conc, negative_ion=negative_ion_conc, temp=temp, want=("binary", "ternary"), stream=stream)
    return r.binary, r.ternary


def organic_nucleation_rate(negative_ion_conc, monoterpene_conc, O3_conc, OH_conc, temp, condensation_sink, params, *, stream=None):
    """Nucleation.organic_nucleation_rate (Nucleation.jl:106-135), Kirkby et al. (2016)."""
    return nucleation_rates(None, params, negative_ion=negative_ion_conc, monoterpene=monoterpene_conc, O3=O3_conc, OH=OH_conc, temp=temp,
                            condensation_sink=condensation_sink, want=("organic",), stream=stream).organic


def organic_and_h2so4_nucleation_rate(h2so4_conc, monoterpene_conc, OH_conc, temp, condensation_sink, params, *, stream=None):
    """Nucleation.organic_and_h2so4_nucleation_rate (Nucleation.jl:172-190), Riccobono et al. (2014)."""
    return nucleation_rates(None, None, params, h2so4=h2so4_conc, monoterpene=monoterpene_conc, OH=OH_conc, temp=temp,
                            condensation_sink=condensation_sink, want=("mixed",), stream=stream).mixed


def nucleation_rates_prescribed(organic_params=None, mixed_params=None, *, negative_ion=None, HOM=None, h2so4=None, bioOxOrg=None,
                                want=("organic", "mixed"), stream=None) -> PrescribedNucleationRates:
    """`cmx_nucleation_rates_prescribed_*`: organic_nucleation_rate_hom_prescribed (:137-157; HOM in cm⁻³, negative_ion as the function receives it)
    and organic_and_h2so4_nucleation_rate_bioOxOrg_prescribed (:192-206; bioOxOrg in m⁻³)."""
    want = tuple(want)
    unknown = set(want) - set(PrescribedNucleationRates._fields)
    if unknown or not want:
        raise ValueError(f"want must name some of {PrescribedNucleationRates._fields}, got {want!r}")
    names = ("negative_ion", "HOM", "h2so4", "bioOxOrg")
    cols = (negative_ion, HOM, h2so4, bioOxOrg)
    need = ({"negative_ion", "HOM"} if "organic" in want else set()) | ({"h2so4", "bioOxOrg"} if "mixed" in want else set())
    missing = [n for n, c in zip(names, cols) if n in need and c is None]
    if missing:
        raise ValueError(f"column(s) {missing} needed for {want}")
    ref, fam = _cols(cols, names)
    op = _need(organic_params, fam.organic_nucleation, "organic_params") if "organic" in want else None
    mp = _need(mixed_params, fam.mixed_nucleation, "mixed_params") if "mixed" in want else None
    outs = {k: (torch.empty_like(ref) if k in want else None) for k in PrescribedNucleationRates._fields}
    _lib.call("cmx_nucleation_rates_prescribed", fam, ref.device, op, mp, ref.numel(), *[_ptr(c if n in need else None) for n, c in zip(names, cols)],
              _ptr(outs["organic"]), _ptr(outs["mixed"]), stream=stream)
    return PrescribedNucleationRates(outs["organic"], outs["mixed"])


def organic_nucleation_rate_hom_prescribed(negative_ion_conc, HOM_conc, params, *, stream=None):
    """Nucleation.organic_nucleation_rate_hom_prescribed (Nucleation.jl:137-157)."""
    return nucleation_rates_prescribed(params, negative_ion=negative_ion_conc, HOM=HOM_conc, want=("organic",), stream=stream).organic


def organic_and_h2so4_nucleation_rate_bioOxOrg_prescribed(h2so4_conc, bioOxOrg, params, *, stream=None):
    """Nucleation.organic_and_h2so4_nucleation_rate_bioOxOrg_prescribed (Nucleation.jl:192-206)."""
    return nucleation_rates_prescribed(None, params, h2so4=h2so4_conc, bioOxOrg=bioOxOrg, want=("mixed",), stream=stream).mixed


def apparent_nucleation_rate(output_diam, nucleation_rate, condensation_growth_rate, coag_sink, coag_sink_input_diam, input_diam=None, *, stream=None):
    """Nucleation.apparent_nucleation_rate (Nucleation.jl:23-37), Lehtinen et al. (2007).  input_diam None: the reference's default 1.7."""
    cols = (output_diam, nucleation_rate, condensation_growth_rate, coag_sink, coag_sink_input_diam, input_diam)
    names = ("output_diam", "nucleation_rate", "condensation_growth_rate", "coag_sink", "coag_sink_input_diam", "input_diam")
    if any(c is None for c in cols[:5]):
        raise ValueError("every column but input_diam is required")
    ref, fam = _cols(cols, names)
    J = torch.empty_like(ref)
    _lib.call("cmx_apparent_nucleation_rate", fam, ref.device, ref.numel(), *[_ptr(c) for c in cols], _ptr(J), stream=stream)
    return J
