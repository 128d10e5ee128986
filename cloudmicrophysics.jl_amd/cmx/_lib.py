"""Loader for libcmx.so (the C-ABI shared library, include/cmx.h) and the one way the wrappers call it.

There is no fallback: if the HIP extension is missing or fails to load, every
product entry point raises `CmxLibraryError`.  Build it with
`python __graft_entry__.py build` (or `make -C cloudmicrophysics.jl_amd/csrc`).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch

from . import _abi

CSRC_DIR = Path(__file__).resolve().parent.parent / "csrc"
LIB_PATH = Path(os.environ.get("CMX_LIB", CSRC_DIR / "libcmx.so"))


class CmxLibraryError(RuntimeError):
    pass


class CmxStatusError(RuntimeError):
    def __init__(self, fn, status, detail=""):
        self.status = status
        names = {_abi.CMX_ERR_BAD_ARG: "CMX_ERR_BAD_ARG", _abi.CMX_ERR_HIP: "CMX_ERR_HIP",
                 _abi.CMX_ERR_UNSUPPORTED: "CMX_ERR_UNSUPPORTED"}
        super().__init__(f"{fn} returned {names.get(status, status)}{': ' + detail if detail else ''}")


_lib = None

_FP = {"f32": C.POINTER(C.c_float), "f64": C.POINTER(C.c_double)}


def _declare(lib):
    vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    lib.cmx_version.restype = i32
    lib.cmx_version.argtypes = []
    lib.cmx_last_hip_error.restype = C.c_char_p
    lib.cmx_last_hip_error.argtypes = []
    lib.cmx_lean_eval_f64.restype = i32
    lib.cmx_lean_eval_f64.argtypes = [i32, i64, vp, vp, vp]
    lib.cmx_lean_eval_literal_f64.restype = i32
    lib.cmx_lean_eval_literal_f64.argtypes = [i32, i64, vp, vp, vp]
    for fam in (_abi.F32, _abi.F64):
        s = fam.sfx
        f = getattr(lib, f"cmx_sb2006_warm_rain_tendencies_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.thermo), C.POINTER(fam.rain_vel), u32, i64] + [vp] * 13 + [vp]
        f = getattr(lib, f"cmx_sb2006_process_rates_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.thermo), C.POINTER(fam.rain_vel), u32, i64] + [vp] * 7 + [
            C.POINTER(vp), vp]
        f = getattr(lib, f"cmx_ice_nucleation_rates_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.thermo), C.POINTER(fam.abifm_dust), C.POINTER(fam.koop2000), u32, i64] + [vp] * 8 + [vp, vp]
        f = getattr(lib, f"cmx_water_activity_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.thermo), i64] + [vp] * 4 + [vp]
        f = getattr(lib, f"cmx_ice_nucleation_rates_xT_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.thermo), C.POINTER(fam.abifm_dust), C.POINTER(fam.koop2000), C.POINTER(fam.h2so4_solution_params), u32, i64] + [vp] * 8 \
            + [vp, vp]
        f = getattr(lib, f"cmx_h2so4_solution_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.h2so4_solution_params), C.POINTER(fam.thermo), i64] + [vp] * 4 + [vp]
        f = getattr(lib, f"cmx_mohler2006_deposition_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.mohler_dust), C.POINTER(fam.mohler2006), i64] + [vp] * 7 + [vp]
        f = getattr(lib, f"cmx_deposition_J_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.deposition_dust), i64, vp, vp, vp]
        f = getattr(lib, f"cmx_inp_concentration_frequency_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.frostenberg2023), i64, vp, vp, vp, vp]
        f = getattr(lib, f"cmx_arg2000_total_activated_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.aerosol_activation_params), C.POINTER(fam.aerosol_distribution), C.POINTER(fam.air_properties),
                      C.POINTER(fam.thermo), i64] + [vp] * 8 + [vp, vp, vp]
        f = getattr(lib, f"cmx_mp0m_tendencies_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.parameters_0m), i64] + [vp] * 5 + [vp]
        f = getattr(lib, f"cmx_mp1m_tendencies_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.thermo), u32, i64] + [vp] * 11 + [vp]
        f = getattr(lib, f"cmx_bulk_2m_cloud_to_rain_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.bulk_2m_schemes), u32, i64] + [vp] * 6 + [vp]
        f = getattr(lib, f"cmx_sedimentation_velocities_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.stokes_vel), C.POINTER(fam.chen2022_rain_vel),
                      C.POINTER(fam.chen2022_ice_vel), i64] + [vp] * 9 + [vp]
        f = getattr(lib, f"cmx_snow_terminal_velocity_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.chen2022_ice_vel), u32, i64] + [vp] * 3 + [vp]
        f = getattr(lib, f"cmx_arg2000_activation_columns_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.aerosol_activation_params), C.POINTER(fam.air_properties), C.POINTER(fam.thermo), i32, i64] \
            + [vp] * 8 + [vp] * 5 + [vp] * 3 + [vp]
        f = getattr(lib, f"cmx_sb2006_cloud_terminal_velocity_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.cloud_pdf_sb2006), C.POINTER(fam.stokes_vel), i64] + [vp] * 5 + [vp]
        f = getattr(lib, f"cmx_sb2006_column_tendencies_sedimentation_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.thermo), C.POINTER(fam.rain_vel), C.POINTER(fam.stokes_vel), u32, i64, i32] \
            + [vp] * 13 + [vp]
        f = getattr(lib, f"cmx_mp1m_linearized_average_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.thermo), u32, fam.ft, fam.ft, i32, i64] + [vp] * 11 + [vp]
        f = getattr(lib, f"cmx_mp1m_source_terms_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.thermo), u32, i64] + [vp] * 7 + [C.POINTER(vp), vp]
        f = getattr(lib, f"cmx_mp1m_terminal_velocity_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.chen2022_rain_vel), i64] + [vp] * 6 + [vp]
        f = getattr(lib, f"cmx_arg2000_activation_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.aerosol_activation_params), C.POINTER(fam.aerosol_distribution),
                      C.POINTER(fam.air_properties), C.POINTER(fam.thermo), i64] + [vp] * 8 + [C.POINTER(vp), C.POINTER(vp), vp, vp]
        f = getattr(lib, f"cmx_p3_shape_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.p3_params), u32, i32, i64] + [vp] * 10 + [vp]
        f = getattr(lib, f"cmx_p3_terminal_velocities_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.p3_params), C.POINTER(fam.chen2022_ice_vel), C.POINTER(fam.quadrature), u32, fam.ft, i64] \
            + [vp] * 8 + [vp]
        f = getattr(lib, f"cmx_p3_shape_terminal_velocities_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.p3_params), C.POINTER(fam.chen2022_ice_vel), C.POINTER(fam.quadrature), u32, i32, fam.ft, i64] \
            + [vp] * 10 + [vp]
        f = getattr(lib, f"cmx_p3_ice_melt_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.p3_params), C.POINTER(fam.chen2022_ice_vel), C.POINTER(fam.air_properties), C.POINTER(fam.thermo),
                      C.POINTER(fam.ventilation), C.POINTER(fam.quadrature), u32, fam.ft, i64] + [vp] * 9 + [vp]
        f = getattr(lib, f"cmx_p3_ice_self_collection_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.p3_params), C.POINTER(fam.chen2022_ice_vel), C.POINTER(fam.quadrature), u32, i64] + [vp] * 7 + [vp]
        f = getattr(lib, f"cmx_liquid_freezing_rate_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.p3_ice_params), C.POINTER(fam.thermo), u32, i64] + [vp] * 6 + [vp]
        f = getattr(lib, f"cmx_p3_het_ice_nucleation_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.abifm_dust), C.POINTER(fam.thermo), i64] + [vp] * 7 + [vp]
        f = getattr(lib, f"cmx_p3_liquid_ice_collisions_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.p3_ice_params), C.POINTER(fam.air_properties), C.POINTER(fam.thermo), C.POINTER(fam.quadrature),
                      u32, i64] + [vp] * 11 + [C.POINTER(vp), C.POINTER(vp), vp]
        f = getattr(lib, f"cmx_sb2006_warm_rain_tendencies_fields_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.thermo), u32, i64, i64, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp),
                      C.POINTER(i64), vp, vp]
        f = getattr(lib, f"cmx_mp1m_column_tendencies_sedimentation_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.thermo), C.POINTER(fam.stokes_vel), C.POINTER(fam.chen2022_rain_vel),
                      C.POINTER(fam.chen2022_ice_vel), u32, fam.ft, fam.ft, i32, i64, i32, vp, C.POINTER(vp), C.POINTER(vp), vp, vp, vp]
        f = getattr(lib, f"cmx_mp1m_linearized_average_fields_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.thermo), u32, fam.ft, fam.ft, i32, i64, i64, C.POINTER(vp), C.POINTER(i64),
                      C.POINTER(vp), C.POINTER(i64), vp, vp]
        f = getattr(lib, f"cmx_mp1m_tendencies_fields_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.thermo), u32, i64, i64, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp),
                      C.POINTER(i64), vp, vp]
        f = getattr(lib, f"cmx_microphysics_2m_p3_tendencies_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.p3_ice_params), C.POINTER(fam.thermo), u32, i64] + [vp] * 13 + \
                     [C.POINTER(vp), vp]
        f = getattr(lib, f"cmx_microphysics_2m_p3_tendencies_fields_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.p3_ice_params), C.POINTER(fam.thermo), u32, i64, i64, C.POINTER(vp), C.POINTER(i64),
                      C.POINTER(vp), C.POINTER(i64), vp]
        f = getattr(lib, f"cmx_mp2m_p3_column_tendencies_sedimentation_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.p3_ice_params), C.POINTER(fam.thermo), C.POINTER(fam.rain_vel),
                      C.POINTER(fam.stokes_vel), u32, i32, fam.ft, i64, i32, vp, C.POINTER(vp), C.POINTER(vp)] + [vp] * 5 + [vp]
        # … with backward-Euler sedimentation (include/cmx.h §24): the same list with `double dt` after p
        f = getattr(lib, f"cmx_mp2m_p3_column_implicit_sedimentation_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.p3_ice_params), C.POINTER(fam.thermo), C.POINTER(fam.rain_vel),
                      C.POINTER(fam.stokes_vel), u32, i32, fam.ft, C.c_double, i64, i32, vp, C.POINTER(vp), C.POINTER(vp)] + [vp] * 5 + [vp]
        f = getattr(lib, f"cmx_gamma_inc_{s}")
        f.restype = i32
        f.argtypes = [i64, vp, vp, vp, vp, vp]
        f = getattr(lib, f"cmx_gamma_inc_inv_{s}")
        f.restype = i32
        f.argtypes = [i64, vp, vp, vp, vp, vp]
        f = getattr(lib, f"cmx_generalized_gamma_{s}")
        f.restype = i32
        f.argtypes = [fam.ft, fam.ft, i64, vp, vp, vp, vp, vp, vp]
        f = getattr(lib, f"cmx_exponential_distribution_{s}")
        f.restype = i32
        f.argtypes = [i64, vp, vp, vp, vp, vp, vp]
        f = getattr(lib, f"cmx_sb2006_size_distribution_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.cloud_pdf_sb2006), C.POINTER(fam.rain_pdf_sb2006), u32, fam.ft, i64] + [vp] * 7 + [vp]
        f = getattr(lib, f"cmx_cloud_diagnostics_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.rain), C.POINTER(fam.cloud_pdf_sb2006), C.POINTER(fam.rain_pdf_sb2006), fam.ft, u32, i64] + [vp] * 9 + [vp]
        f = getattr(lib, f"cmx_aerosol_nucleation_rates_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.h2so4_nucleation), C.POINTER(fam.organic_nucleation), C.POINTER(fam.mixed_nucleation), i64] + [vp] * 12 + [vp]
        f = getattr(lib, f"cmx_nucleation_rates_prescribed_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.organic_nucleation), C.POINTER(fam.mixed_nucleation), i64] + [vp] * 6 + [vp]
        f = getattr(lib, f"cmx_apparent_nucleation_rate_{s}")
        f.restype = i32
        f.argtypes = [i64] + [vp] * 7 + [vp]
        f = getattr(lib, f"cmx_p3_ice_nucleation_counts_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.morrison_milbrandt2014), i64] + [vp] * 6 + [vp]
        f = getattr(lib, f"cmx_sb2006_precip_susceptibility_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.acnv_sb2006), C.POINTER(fam.accr_sb2006), i64] + [vp] * 10 + [vp]
        f = getattr(lib, f"cmx_sb2006_warm_rain_jacobian_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.thermo), u32, i64] + [vp] * 7 + [C.POINTER(vp), C.POINTER(vp), vp]
        f = getattr(lib, f"cmx_mp1m_jacobian_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.thermo), u32, i64] + [vp] * 7 + [C.POINTER(vp), C.POINTER(vp), vp]
        for stem, params in (("cmx_sb2006_warm_rain", fam.warm_rain_2m), ("cmx_mp1m", fam.microphysics_1m)):
            for product in ("jvp", "vjp"):       # (tangents[6], jvp[4], tendencies[4]) / (cotangents[4], grad[6], tendencies[4])
                f = getattr(lib, f"{stem}_{product}_{s}")
                f.restype = i32
                f.argtypes = [C.POINTER(params), C.POINTER(fam.thermo), u32, i64] + [vp] * 7 + [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]
            f = getattr(lib, f"{stem}_implicit_tendencies_{s}")       # (dt, implicit[4], tendencies[4])
            f.restype = i32
            f.argtypes = [C.POINTER(params), C.POINTER(fam.thermo), u32, i64] + [vp] * 7 + [C.c_double, C.POINTER(vp), C.POINTER(vp), vp]
            f = getattr(lib, f"{stem}_implicit_average_{s}")          # (dt, nsub, step_flags, average[4])
            f.restype = i32
            f.argtypes = [C.POINTER(params), C.POINTER(fam.thermo), u32, i64] + [vp] * 7 + [C.c_double, i32, u32, C.POINTER(vp), vp]
        # the derivatives with respect to the parameters (include/cmx.h §22): (…state…, ndir, d_warm_rain, d_tps, jvp[ndir·4], tendencies[4]) /
        # (…state…, cotangents[4], ndir, d_warm_rain, d_tps, grad, workspace, tendencies[4])
        for stem, params in (("cmx_sb2006_warm_rain", fam.warm_rain_2m), ("cmx_mp1m", fam.microphysics_1m)):      # §22, §23
            f = getattr(lib, f"{stem}_param_jvp_{s}")
            f.restype = i32
            f.argtypes = [C.POINTER(params), C.POINTER(fam.thermo), u32, i64] + [vp] * 7 + [i32, C.POINTER(params), C.POINTER(fam.thermo), C.POINTER(vp),
                                                                                           C.POINTER(vp), vp]
            f = getattr(lib, f"{stem}_param_vjp_{s}")
            f.restype = i32
            f.argtypes = [C.POINTER(params), C.POINTER(fam.thermo), u32, i64] + [vp] * 7 + [C.POINTER(vp), i32, C.POINTER(params), C.POINTER(fam.thermo), vp, vp,
                                                                                           C.POINTER(vp), vp]
        # the column steps with the implicit average as tendency (include/cmx.h §20): (flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, …)
        # … and with backward-Euler sedimentation (§21): the same argument lists
        for step in ("implicit_average_sedimentation", "implicit_step"):
            f = getattr(lib, f"cmx_sb2006_column_{step}_{s}")
            f.restype = i32
            f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.thermo), C.POINTER(fam.rain_vel), C.POINTER(fam.stokes_vel), u32, C.c_double, i32, u32,
                          i64, i32] + [vp] * 13 + [vp]
            f = getattr(lib, f"cmx_mp1m_column_{step}_{s}")
            f.restype = i32
            f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.thermo), C.POINTER(fam.stokes_vel), C.POINTER(fam.chen2022_rain_vel),
                          C.POINTER(fam.chen2022_ice_vel), u32, C.c_double, i32, u32, i64, i32, vp, C.POINTER(vp), C.POINTER(vp), vp, vp, vp]
        # J v and Jᵀḡ of the SB2006 column step (include/cmx.h §25): the head of cmx_sb2006_column_tendencies_sedimentation_* through n_rai, then
        # (tangents[6], jvp[4], jvp_precip, tendencies[4], precip_flux) / (cotangents[4], cot_precip, grad[6], tendencies[4], precip_flux)
        head = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.thermo), C.POINTER(fam.rain_vel), C.POINTER(fam.stokes_vel), u32, i64, i32] + [vp] * 8
        f = getattr(lib, f"cmx_sb2006_column_jvp_{s}")
        f.restype = i32
        f.argtypes = head + [C.POINTER(vp), C.POINTER(vp), vp, C.POINTER(vp), vp, vp]
        f = getattr(lib, f"cmx_sb2006_column_vjp_{s}")
        f.restype = i32
        f.argtypes = head + [C.POINTER(vp), vp, C.POINTER(vp), C.POINTER(vp), vp, vp]
        # the derivatives of the same step with respect to the parameters (include/cmx.h §26): the same head, then
        # (ndir, d_warm_rain, d_tps, d_vel, d_cloud_vel, jvp[ndir·4], jvp_precip[ndir], tendencies[4], precip_flux) /
        # (cotangents[4], cot_precip, ndir, d_warm_rain, d_tps, d_vel, d_cloud_vel, grad, workspace, tendencies[4], precip_flux)
        dirs = [i32, C.POINTER(fam.warm_rain_2m), C.POINTER(fam.thermo), C.POINTER(fam.rain_vel), C.POINTER(fam.stokes_vel)]
        f = getattr(lib, f"cmx_sb2006_column_param_jvp_{s}")
        f.restype = i32
        f.argtypes = head + dirs + [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp]
        f = getattr(lib, f"cmx_sb2006_column_param_vjp_{s}")
        f.restype = i32
        f.argtypes = head + [C.POINTER(vp), vp] + dirs + [vp, vp, C.POINTER(vp), vp, vp]
        # J v and Jᵀḡ of the 1-moment column step (include/cmx.h §27): the head of cmx_mp1m_column_tendencies_sedimentation_* through `in` without q_min, dt,
        # nsub, then (tangents[6], jvp[4], jvp_precip_rai, jvp_precip_sno, tendencies[4], precip_rai, precip_sno) /
        # (cotangents[4], cot_precip_rai, cot_precip_sno, grad[6], tendencies[4], precip_rai, precip_sno)
        head = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.thermo), C.POINTER(fam.stokes_vel), C.POINTER(fam.chen2022_rain_vel),
                C.POINTER(fam.chen2022_ice_vel), u32, i64, i32, vp, C.POINTER(vp)]
        f = getattr(lib, f"cmx_mp1m_column_jvp_{s}")
        f.restype = i32
        f.argtypes = head + [C.POINTER(vp), C.POINTER(vp), vp, vp, C.POINTER(vp), vp, vp, vp]
        f = getattr(lib, f"cmx_mp1m_column_vjp_{s}")
        f.restype = i32
        f.argtypes = head + [C.POINTER(vp), vp, vp, C.POINTER(vp), C.POINTER(vp), vp, vp, vp]
        # the derivatives of the same step with respect to the parameters (include/cmx.h §28): the same head, then
        # (ndir, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice, jvp[ndir·4], jvp_precip_rai[ndir], jvp_precip_sno[ndir], tendencies[4], precip_rai, precip_sno) /
        # (cotangents[4], cot_precip_rai, cot_precip_sno, ndir, the five direction tables, grad, workspace, tendencies[4], precip_rai, precip_sno)
        dirs = [i32] + head[:5]
        f = getattr(lib, f"cmx_mp1m_column_param_jvp_{s}")
        f.restype = i32
        f.argtypes = head + dirs + [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, vp]
        f = getattr(lib, f"cmx_mp1m_column_param_vjp_{s}")
        f.restype = i32
        f.argtypes = head + [C.POINTER(vp), vp, vp] + dirs + [vp, vp, C.POINTER(vp), vp, vp, vp]
        f = getattr(lib, f"cmx_parcel_tendencies_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.parcel_params), u32, i64, C.POINTER(vp), vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]
        f = getattr(lib, f"cmx_parcel_run_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.parcel_params), u32, i64, i64, i64, C.POINTER(vp), vp, C.POINTER(vp), C.POINTER(vp), vp, vp]
        f = getattr(lib, f"cmx_column_sums_{s}")
        f.restype = i32
        f.argtypes = [i32, C.POINTER(vp), i64, vp, vp, vp]
        # parameter ensembles (include/cmx.h §29): pack (arrays of parameter structs, flags, n_members, host table, table_bytes, desc), then the ensemble
        # entries: (desc, device table, n_members, ens_flags) in front of the single entry's array arguments
        desc = C.POINTER(_abi.EnsembleDesc)
        for scheme in ("sb2006", "mp1m"):
            f = getattr(lib, f"cmx_{scheme}_ensemble_table_stride_{s}")
            f.restype = i32
            f.argtypes = []
        f = getattr(lib, f"cmx_sb2006_ensemble_pack_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.warm_rain_2m), C.POINTER(fam.thermo), C.POINTER(fam.rain_vel), C.POINTER(fam.stokes_vel), u32, i32, vp, i64, desc]
        f = getattr(lib, f"cmx_mp1m_ensemble_pack_{s}")
        f.restype = i32
        f.argtypes = [C.POINTER(fam.microphysics_1m), C.POINTER(fam.thermo), C.POINTER(fam.stokes_vel), C.POINTER(fam.chen2022_rain_vel),
                      C.POINTER(fam.chen2022_ice_vel), u32, i32, vp, i64, desc]
        f = getattr(lib, f"cmx_sb2006_warm_rain_tendencies_ensemble_{s}")
        f.restype = i32
        f.argtypes = [desc, vp, i32, u32, i64] + [vp] * 13 + [vp]
        f = getattr(lib, f"cmx_mp1m_tendencies_ensemble_{s}")
        f.restype = i32
        f.argtypes = [desc, vp, i32, u32, i64] + [vp] * 11 + [vp]
        f = getattr(lib, f"cmx_sb2006_column_tendencies_sedimentation_ensemble_{s}")
        f.restype = i32
        f.argtypes = [desc, vp, i32, u32, i64, i32] + [vp] * 13 + [vp]
        f = getattr(lib, f"cmx_mp1m_column_tendencies_sedimentation_ensemble_{s}")
        f.restype = i32
        f.argtypes = [desc, vp, i32, u32, fam.ft, fam.ft, i32, i64, i32, vp, C.POINTER(vp), C.POINTER(vp), vp, vp, vp]
        # … of the implicit column steps (§21): (desc, device table, n_members, ens_flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, …)
        f = getattr(lib, f"cmx_sb2006_column_implicit_step_ensemble_{s}")
        f.restype = i32
        f.argtypes = [desc, vp, i32, u32, C.c_double, i32, u32, i64, i32] + [vp] * 13 + [vp]
        f = getattr(lib, f"cmx_mp1m_column_implicit_step_ensemble_{s}")
        f.restype = i32
        f.argtypes = [desc, vp, i32, u32, C.c_double, i32, u32, i64, i32, vp, C.POINTER(vp), C.POINTER(vp), vp, vp, vp]


def lib():
    """The loaded library; raises CmxLibraryError (never falls back) if it is unavailable."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise CmxLibraryError(
                f"{LIB_PATH} not found: the HIP extension is not built. "
                "Run `python __graft_entry__.py build` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        try:
            handle = C.CDLL(str(LIB_PATH))
        except OSError as e:  # missing libamdhip64 etc.
            raise CmxLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        _declare(handle)
        _lib = handle
    return _lib


def check(fn_name, status):
    if status < 0:
        detail = lib().cmx_last_hip_error().decode() if status == _abi.CMX_ERR_HIP else ""
        raise CmxStatusError(fn_name, status, detail)
    return status


def call(stem, fam, device, *args, stream=None):
    """Calls `{stem}_{fam.sfx}`(*args, stream) on `device` (stream: the device's current stream by default) and raises
    CmxStatusError if it fails.  Nothing else: the wrappers are captured into graphs (tests/test_graphs_gpu.py)."""
    fn = getattr(lib(), f"{stem}_{fam.sfx}")
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.device(device):
        st = fn(*args, C.c_void_p(s.cuda_stream))
    return check(fn.__name__, st)

