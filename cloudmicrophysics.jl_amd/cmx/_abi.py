"""ctypes mirror of include/cmx.h (structs, flags, column ids).

One factory stamps the Float32 and the Float64 struct family, exactly like the
CMX_DECLARE_PARAM_STRUCTS macro of the header.  Field order is the declaration
order of the reference's Julia structs (cited in include/cmx.h).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

# ---- flags (include/cmx.h) ---------------------------------------------------
CMX_SB2006_LIMITED = 1 << 0
CMX_VEL_SB2006 = 1 << 1
CMX_VEL_CHEN2022 = 1 << 2

CMX_ARG_MAX_MODES = 8
CMX_2M_KK2000, CMX_2M_B1994, CMX_2M_TC1980, CMX_2M_LD2004 = 0, 1, 2, 3
CMX_2M_SMOOTH_TRANSITION = 1 << 8
CMX_P3_INPUT_IS_STATE = 1 << 0
CMX_P3_SLOPE_CONSTANT = 1 << 1
CMX_P3_NO_ASPECT_RATIO = 1 << 2
CMX_P3_RAIN_PDF_LIMITED = 1 << 3
CMX_FREEZE_CLOUD_PSD = 1 << 4
CMX_P3COL_VEL_SB2006 = 1 << 8      # cmx_mp2m_p3_column_tendencies_sedimentation_*: the rain fall-speed scheme (bits 1, 2 are P3 flags there)
CMX_P3COL_VEL_CHEN2022 = 1 << 9
CMX_QUAD_MAX = 128
CMX_PSD_CLOUD = 1 << 5
CMX_COLUMN_SUMS_MAX_COLS = 16
CMX_COLUMN_SUMS_PARTIALS = 1024

CMX_ICENUC_HOM_LINEAR = 1 << 0
CMX_ICENUC_ERR_SLOTS = 64
CMX_ICENUC_ERR_WORDS = 1024

# Microphysics1MOptions bits (include/cmx.h §5)
CMX_1M_CLOUD_LIQUID_FORMATION = 1 << 0
CMX_1M_CLOUD_ICE_FORMATION_CONST = 1 << 1
CMX_1M_CLOUD_ICE_FORMATION_TDEP = 1 << 2
CMX_1M_CLOUD_ICE_MELT = 1 << 3
CMX_1M_RAIN_ACNV_KESSLER = 1 << 4
CMX_1M_RAIN_ACNV_PRESCRIBED_ND = 1 << 5
CMX_1M_SNOW_ACNV_NO_SUPERSAT = 1 << 6
CMX_1M_SNOW_ACNV_WITH_SUPERSAT = 1 << 7
CMX_1M_RAIN_EVAPORATION = 1 << 8
CMX_1M_SNOW_SUBLIMATION_ONLY = 1 << 9
CMX_1M_SNOW_DEP_AND_SUBL = 1 << 10
CMX_1M_SNOW_MELT = 1 << 11
CMX_1M_ACCR_LCL_RAI = 1 << 12
CMX_1M_ACCR_LCL_SNO = 1 << 13
CMX_1M_ACCR_ICL_RAI = 1 << 14
CMX_1M_ACCR_ICL_SNO = 1 << 15
CMX_1M_ACCR_RAI_SNO = 1 << 16
CMX_1M_DEFAULT_OPTIONS = (CMX_1M_CLOUD_LIQUID_FORMATION | CMX_1M_CLOUD_ICE_FORMATION_CONST | CMX_1M_CLOUD_ICE_MELT |
                          CMX_1M_RAIN_ACNV_KESSLER | CMX_1M_SNOW_ACNV_NO_SUPERSAT | CMX_1M_RAIN_EVAPORATION |
                          CMX_1M_SNOW_DEP_AND_SUBL | CMX_1M_SNOW_MELT | CMX_1M_ACCR_LCL_RAI | CMX_1M_ACCR_LCL_SNO |
                          CMX_1M_ACCR_ICL_RAI | CMX_1M_ACCR_ICL_SNO | CMX_1M_ACCR_RAI_SNO)
# snow shape of the Chen-2022 snow fall speed: cmx_snow_terminal_velocity_* `snow_shape`; CMX_1M_SED_SNOW_* — column step only
CMX_SNOW_SHAPE_ASPR = 0
CMX_SNOW_SHAPE_OBLATE = 1
CMX_SNOW_SHAPE_PROLATE = 2
CMX_1M_SED_SNOW_OBLATE = 1 << 17
CMX_1M_SED_SNOW_PROLATE = 1 << 18

# cmx_mp1m_source_column
MP1M_SOURCE_COLUMNS = (
    "S_phase_change_vap_lcl", "S_phase_change_vap_icl", "S_acnv_lcl_rai", "S_acnv_icl_sno",
    "S_accr_lcl_rai", "S_accr_lcl_sno_cold", "S_accr_lcl_sno_warm", "S_accr_melt_lcl_sno",
    "S_accr_icl_rai", "S_accr_freeze_icl_rai", "S_accr_icl_sno",
    "S_accr_rai_sno_cold", "S_accr_rai_sno_warm", "S_accr_melt_rai_sno",
    "S_phase_change_vap_rai", "S_phase_change_vap_sno", "S_melt_icl_lcl", "S_melt_sno_rai",
)
CMX_MP1M_NSRC = len(MP1M_SOURCE_COLUMNS)

# the parcel model (include/cmx.h §13): one field of the flags word per member of the reference's parcel_params
CMX_PARCEL_AERO_ACT = 1 << 0
CMX_PARCEL_DEP_MASK = 7 << 4
CMX_PARCEL_DEP_MOHLER_AF = 1 << 4
CMX_PARCEL_DEP_MOHLER_RATE = 2 << 4
CMX_PARCEL_DEP_ABDINM = 3 << 4
CMX_PARCEL_DEP_P3 = 4 << 4
CMX_PARCEL_HET_MASK = 7 << 8
CMX_PARCEL_HET_ABIFM = 1 << 8
CMX_PARCEL_HET_P3 = 2 << 8
CMX_PARCEL_HET_FROSTENBERG_RANDOM = 3 << 8
CMX_PARCEL_HET_FROSTENBERG_MEAN = 4 << 8
CMX_PARCEL_HET_FROSTENBERG_STOCHASTIC = 5 << 8
CMX_PARCEL_HOM_MASK = 3 << 12
CMX_PARCEL_HOM_ABHOM = 1 << 12
CMX_PARCEL_HOM_P3 = 2 << 12
CMX_PARCEL_COND_MASK = 3 << 16
CMX_PARCEL_COND_CONDENSATION = 1 << 16
CMX_PARCEL_COND_NONEQ_SIMPLE = 2 << 16
CMX_PARCEL_COND_NONEQ = 3 << 16
CMX_PARCEL_DEPGROWTH_MASK = 3 << 20
CMX_PARCEL_DEPGROWTH_DEPOSITION = 1 << 20
CMX_PARCEL_DEPGROWTH_NONEQ_SIMPLE = 2 << 20
CMX_PARCEL_DEPGROWTH_NONEQ = 3 << 20
CMX_PARCEL_LIQ_MASK = 3 << 24
CMX_PARCEL_LIQ_GAMMA = 1 << 24
CMX_PARCEL_LIQ_MONODISPERSE_MIX = 2 << 24
CMX_PARCEL_ICE_GAMMA = 1 << 26
CMX_PARCEL_PRESCRIBED_THERMODYNAMICS = 1 << 28
CMX_PARCEL_NSTATE = 9
CMX_PARCEL_NCOEF = 6
CMX_PARCEL_NPROC = 6
CMX_PARCEL_MAX_STEPS_PER_LAUNCH = 256
PARCEL_STATE_COLUMNS = ("S_l", "p_air", "T", "q_vap", "q_liq", "q_ice", "N_aer", "N_liq", "N_ice")
PARCEL_PROCESS_COLUMNS = ("dN_liq_act", "dN_ice_dep", "dN_ice_imm", "dN_ice_hom", "dq_liq_ce", "dq_ice_ds")
PARCEL_COEFFICIENT_COLUMNS = ("deposition_m", "deposition_c", "ABIFM_m", "ABIFM_c", "linear_c1", "linear_c2")

CMX_OK = 0
CMX_ERR_BAD_ARG = -1
CMX_ERR_HIP = -2
CMX_ERR_UNSUPPORTED = -3

# cmx_sb2006_process_column
SB2006_PROCESS_COLUMNS = (
    "acnv_dq_lcl_dt", "acnv_dN_lcl_dt", "acnv_dq_rai_dt", "acnv_dN_rai_dt",
    "lcl_self_collection",
    "accr_dq_lcl_dt", "accr_dN_lcl_dt", "accr_dq_rai_dt",
    "rain_self_collection", "rain_breakup",
    "rain_vel_n", "rain_vel_m",
    "evap_dN_rai_dt", "evap_dq_rai_dt",
    "numadj_rai", "numadj_lcl",
    "condevap",
    "devap_dN_rai", "devap_dq_rai",
)
CMX_SB2006_NPROC = len(SB2006_PROCESS_COLUMNS)

# cmx_sb2006_jac_out, cmx_sb2006_jac_wrt (include/cmx.h §14): jac[o * CMX_SB2006_JAC_NWRT + i] = ∂out_o/∂in_i
SB2006_JAC_OUT = ("dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt")
SB2006_JAC_WRT = ("T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai")
CMX_SB2006_JAC_NOUT = len(SB2006_JAC_OUT)
CMX_SB2006_JAC_NWRT = len(SB2006_JAC_WRT)
CMX_SB2006_JAC_NCOL = CMX_SB2006_JAC_NOUT * CMX_SB2006_JAC_NWRT

# cmx_mp1m_jac_out, cmx_mp1m_jac_wrt (include/cmx.h §15): jac[o * CMX_MP1M_JAC_NWRT + i] = ∂out_o/∂in_i
MP1M_JAC_OUT = ("dq_lcl_dt", "dq_icl_dt", "dq_rai_dt", "dq_sno_dt")
MP1M_JAC_WRT = ("T", "q_tot", "q_lcl", "q_icl", "q_rai", "q_sno")
CMX_MP1M_JAC_NOUT = len(MP1M_JAC_OUT)
CMX_MP1M_JAC_NWRT = len(MP1M_JAC_WRT)
CMX_MP1M_JAC_NCOL = CMX_MP1M_JAC_NOUT * CMX_MP1M_JAC_NWRT

# the products with the two Jacobians (include/cmx.h §16, §17): <stem>_jvp_* takes tangents[NWRT], jvp[NOUT], tendencies[NOUT]; <stem>_vjp_* takes
# cotangents[NOUT], grad[NWRT], tendencies[NOUT]
JACOBIAN_PRODUCT_STEMS = ("cmx_sb2006_warm_rain", "cmx_mp1m")
# the linearly implicit tendencies of the same two schemes (include/cmx.h §18): <stem>_implicit_tendencies_* takes dt, implicit[NOUT], tendencies[NOUT]
# … and their average over nsub substeps (include/cmx.h §19): <stem>_implicit_average_* takes dt, nsub, step_flags, average[NOUT]
CMX_STEP_NONNEGATIVE = 1
CMX_IMPLICIT_AVERAGE_MAX_NSUB = 64
# … and as tendency operator of the column steps (include/cmx.h §20): cmx_<scheme>_column_implicit_average_sedimentation_* take the same dt, nsub, step_flags
# … and with backward-Euler sedimentation (include/cmx.h §21): cmx_<scheme>_column_implicit_step_*, the argument lists of §20
# the 2M + P3 column step with backward-Euler sedimentation (include/cmx.h §24): cmx_mp2m_p3_column_implicit_sedimentation_* takes the argument list of
# cmx_mp2m_p3_column_tendencies_sedimentation_* (9b) with one `double dt` (≥ 0) after p, and the flag bits CMX_P3COL_VEL_* of that entry
# J v and Jᵀḡ of the SB2006 column step with sedimentation (include/cmx.h §25): cmx_sb2006_column_jvp_* / _vjp_* take the head of
# cmx_sb2006_column_tendencies_sedimentation_* through n_rai, then tangents[NWRT], jvp[NOUT], jvp_precip, tendencies[NOUT], precip_flux resp.
# cotangents[NOUT], cot_precip, grad[NWRT], tendencies[NOUT], precip_flux, in the orders of SB2006_JAC_WRT / SB2006_JAC_OUT
# … and its derivatives with respect to the parameters (include/cmx.h §26): cmx_sb2006_column_param_jvp_* / _param_vjp_* take the same head, then ndir,
# d_warm_rain, d_tps, d_vel, d_cloud_vel, jvp[ndir·NOUT], jvp_precip[ndir], tendencies[NOUT], precip_flux resp. cotangents[NOUT], cot_precip, ndir, the four
# direction tables, grad (ndir doubles), workspace (ndir·CMX_PARAM_VJP_PARTIALS doubles), tendencies[NOUT], precip_flux
# J v and Jᵀḡ of the 1-moment column step with sedimentation (include/cmx.h §27): cmx_mp1m_column_jvp_* / _vjp_* take the head of
# cmx_mp1m_column_tendencies_sedimentation_* through `in` without q_min, dt, nsub (Instantaneous mode), then tangents[NWRT], jvp[NOUT], jvp_precip_rai,
# jvp_precip_sno, tendencies[NOUT], precip_rai, precip_sno resp. cotangents[NOUT], cot_precip_rai, cot_precip_sno, grad[NWRT], tendencies[NOUT], precip_rai,
# precip_sno, in the orders of MP1M_JAC_WRT / MP1M_JAC_OUT
# … and its derivatives with respect to the parameters (include/cmx.h §28): cmx_mp1m_column_param_jvp_* / _param_vjp_* take the same head, then ndir, d_mp,
# d_tps, d_stokes, d_chen_rain, d_chen_ice, jvp[ndir·NOUT], jvp_precip_rai[ndir], jvp_precip_sno[ndir], tendencies[NOUT], precip_rai, precip_sno resp.
# cotangents[NOUT], cot_precip_rai, cot_precip_sno, ndir, the five direction tables, grad (ndir doubles), workspace (ndir·CMX_PARAM_VJP_PARTIALS doubles),
# tendencies[NOUT], precip_rai, precip_sno
# the derivatives with respect to the parameters (include/cmx.h §22, §23: cmx_mp1m_param_jvp_* / _param_vjp_* take the same lists over cmx_microphysics_1m): cmx_sb2006_warm_rain_param_jvp_* takes ndir, d_warm_rain[ndir], d_tps[ndir], jvp[ndir·NOUT],
# tendencies[NOUT]; …_param_vjp_* takes cotangents[NOUT], ndir, d_warm_rain, d_tps, grad (ndir doubles), workspace (ndir·CMX_PARAM_VJP_PARTIALS doubles), tendencies
CMX_PARAM_MAX_DIRS = 16
CMX_PARAM_VJP_PARTIALS = 1024

# parameter ensembles (include/cmx.h §29): cmx_<scheme>_ensemble_pack_* fold arrays of parameter structs into a host table and this descriptor; the
# <single entry>_ensemble_* entries take (desc, device table, n_members, ens_flags) in front of the single entry's array arguments
CMX_ENSEMBLE_SHARED_STATE = 1 << 0
CMX_ENSEMBLE_MAGIC = 0x434D5845
CMX_ENSEMBLE_SCHEME_SB2006 = 1
CMX_ENSEMBLE_SCHEME_MP1M = 2
CMX_ENSEMBLE_MAX_MEMBERS = 65535


class EnsembleDesc(C.Structure):
    """cmx_ensemble_desc"""
    _fields_ = [("magic", C.c_uint32), ("scheme", C.c_uint32), ("float_type", C.c_uint32), ("flags", C.c_uint32), ("n_members", C.c_int32),
                ("stride", C.c_uint32), ("integer_exponents", C.c_uint32), ("vel_kind", C.c_uint32), ("cloud_vel", C.c_uint32),
                ("runtime_flags", C.c_uint32), ("sedimentation", C.c_uint32), ("general_gamma", C.c_uint32), ("reserved", C.c_uint32 * 4)]


def _struct(name, fields):
    return type(name, (C.Structure,), {"_fields_": fields})


def _family(ft, sfx):
    s = lambda *names: [(n, ft) for n in names]  # noqa: E731
    ns = SimpleNamespace(ft=ft, sfx=sfx)
    ns.cloud_pdf_sb2006 = _struct(f"cmx_cloud_pdf_sb2006_{sfx}",
                                  s("nu_c", "mu_c", "xc_min", "xc_max", "rho_w", "loggamma_z1", "loggamma_z2"))
    ns.rain_pdf_sb2006 = _struct(f"cmx_rain_pdf_sb2006_{sfx}",
                                 s("nu_r", "mu_r", "xr_min", "xr_max", "N0_min", "N0_max",
                                   "lambda_min", "lambda_max", "rho_w", "rho_0"))
    ns.kk2000 = _struct(f"cmx_kk2000_{sfx}", s("acnv_A", "acnv_a", "acnv_b", "acnv_c", "accr_A", "accr_a", "accr_b"))
    ns.b1994 = _struct(f"cmx_b1994_{sfx}", s("acnv_C", "acnv_a", "acnv_b", "acnv_c", "acnv_N_0", "acnv_d_low", "acnv_d_high", "acnv_k", "accr_A"))
    ns.tc1980 = _struct(f"cmx_tc1980_{sfx}", s("acnv_a", "acnv_b", "acnv_D", "acnv_r_0", "acnv_me_liq", "acnv_m0_liq_coeff", "acnv_k", "accr_A"))
    ns.ld2004 = _struct(f"cmx_ld2004_{sfx}", s("R_6C_0", "E_0", "rho_w", "k"))
    ns.bulk_2m_schemes = _struct(f"cmx_bulk_2m_schemes_{sfx}", [("kk2000", ns.kk2000), ("b1994", ns.b1994), ("tc1980", ns.tc1980),
                                                                  ("ld2004", ns.ld2004)])
    ns.stokes_vel = _struct(f"cmx_stokes_vel_{sfx}", s("rho_w", "nu_air", "grav"))
    ns.acnv_sb2006 = _struct(f"cmx_acnv_sb2006_{sfx}", s("kcc", "x_star", "rho_0", "A", "a", "b"))
    ns.accr_sb2006 = _struct(f"cmx_accr_sb2006_{sfx}", s("kcr", "tau_0", "rho_0", "c"))
    ns.selfcol_sb2006 = _struct(f"cmx_selfcol_sb2006_{sfx}", s("krr", "kappa_rr", "d"))
    ns.breakup_sb2006 = _struct(f"cmx_breakup_sb2006_{sfx}", s("Deq", "Dr_th", "kbr", "kappa_br"))
    ns.evap_sb2006 = _struct(f"cmx_evap_sb2006_{sfx}",
                             s("av", "bv", "alpha", "beta", "rho_0", "a_vent_1", "b_vent_1",
                               "a_vent_0_coeff", "b_vent_0_coeff", "beta_vent_0"))
    ns.numadj_horn2012 = _struct(f"cmx_numadj_horn2012_{sfx}", s("tau"))
    ns.sb2006 = _struct(f"cmx_sb2006_{sfx}", [
        ("pdf_c", ns.cloud_pdf_sb2006), ("pdf_r", ns.rain_pdf_sb2006), ("acnv", ns.acnv_sb2006),
        ("accr", ns.accr_sb2006), ("self", ns.selfcol_sb2006), ("brek", ns.breakup_sb2006),
        ("evap", ns.evap_sb2006), ("numadj", ns.numadj_horn2012)])
    ns.air_properties = _struct(f"cmx_air_properties_{sfx}", s("K_therm", "D_vapor", "nu_air"))
    ns.warm_rain_2m = _struct(f"cmx_warm_rain_2m_{sfx}", [
        ("seifert_beheng", ns.sb2006), ("air_properties", ns.air_properties),
        ("condevap_tau_relax", ft), ("subdep_tau_relax", ft)])
    ns.thermo = _struct(f"cmx_thermo_{sfx}",
                        s("R_v", "R_d", "cp_d", "cp_v", "cp_l", "cp_i", "LH_v0", "LH_s0", "T_0",
                          "T_triple", "press_triple", "T_freeze", "cv_l"))
    ns.sb2006_vel = _struct(f"cmx_sb2006_vel_{sfx}", s("rho_0", "aR", "bR", "cR", "rho_w", "nu_air", "grav"))
    ns.chen2022_rain_vel = _struct(f"cmx_chen2022_rain_vel_{sfx}", [
        ("rho_0", ft), ("a", ft * 3), ("a3_pow", ft), ("b", ft * 3), ("b_rho", ft), ("c", ft * 3)])
    ns.rain_vel = _struct(f"cmx_rain_vel_{sfx}", [("sb2006", ns.sb2006_vel), ("chen2022", ns.chen2022_rain_vel)])
    ns.koop2000 = _struct(f"cmx_koop2000_{sfx}",
                          s("delta_a_w_min", "delta_a_w_max", "c1", "c2", "c3", "c4", "linear_c1", "linear_c2"))
    ns.abifm_dust = _struct(f"cmx_abifm_dust_{sfx}", s("ABIFM_m", "ABIFM_c"))
    # ---- 1-moment scheme
    ns.particle_mass = _struct(f"cmx_particle_mass_{sfx}", s("r0", "m0", "me", "delta_m", "chi_m", "gamma_coeff"))
    ns.particle_area = _struct(f"cmx_particle_area_{sfx}", s("a0", "ae", "delta_a", "chi_a"))
    ns.ventilation = _struct(f"cmx_ventilation_{sfx}", s("a", "b"))
    ns.acnv_1m = _struct(f"cmx_acnv_1m_{sfx}", s("tau", "q_threshold", "k"))
    ns.var_timescale_acnv = _struct(f"cmx_var_timescale_acnv_{sfx}", s("tau", "alpha", "Nc"))
    ns.cloud_liquid = _struct(f"cmx_cloud_liquid_{sfx}", s("rho_w", "r_eff", "N_0"))
    ns.cloud_ice = _struct(f"cmx_cloud_ice_{sfx}", [("n0", ft), ("mass", ns.particle_mass)] + s("rho_i", "r_eff", "N_0"))
    ns.rain = _struct(f"cmx_rain_{sfx}", [("n0", ft), ("mass", ns.particle_mass), ("area", ns.particle_area),
                                          ("vent", ns.ventilation)])
    ns.snow = _struct(f"cmx_snow_{sfx}", s("mu", "nu") + [("mass", ns.particle_mass), ("area", ns.particle_area),
                                                         ("vent", ns.ventilation)] +
                      s("phi", "kappa", "rho_i", "gamma_aspect_oblate", "gamma_aspect_prolate"))
    ns.blk1m_vel_rain = _struct(f"cmx_blk1m_vel_rain_{sfx}",
                                s("r0", "ve", "delta_v", "chi_v", "rho_w", "C_drag", "grav", "gamma_vent", "gamma_term",
                                  "gamma_accr", "gamma_accr_rain_sink"))
    ns.blk1m_vel_snow = _struct(f"cmx_blk1m_vel_snow_{sfx}",
                                s("r0", "ve", "delta_v", "chi_v", "v0", "gamma_vent", "gamma_term", "gamma_accr"))
    ns.frostenberg2023 = _struct(f"cmx_frostenberg2023_{sfx}", s("sigma", "a", "b", "T_freeze", "log_a"))
    ns.process_params_1m = _struct(f"cmx_process_params_1m_{sfx}", s(
        "cloud_liquid_formation_tau_relax", "cloud_ice_formation_tau_relax") + [
        ("cloud_ice_formation_frostenberg", ns.frostenberg2023), ("rain_autoconversion", ns.acnv_1m), ("rain_autoconversion_nd", ns.var_timescale_acnv),
        ("snow_autoconversion", ns.acnv_1m)] + s(
        "r_ice_snow", "e_lcl_rai", "e_lcl_sno", "e_icl_rai", "e_icl_sno", "e_rai_sno", "coeff_disp"))
    ns.microphysics_1m = _struct(f"cmx_microphysics_1m_{sfx}", [
        ("process_params", ns.process_params_1m), ("cloud_liquid", ns.cloud_liquid), ("cloud_ice", ns.cloud_ice),
        ("rain", ns.rain), ("snow", ns.snow), ("air_properties", ns.air_properties),
        ("vel_rain", ns.blk1m_vel_rain), ("vel_snow", ns.blk1m_vel_snow)])
    # ---- ARG2000 aerosol activation
    ns.aerosol_activation_params = _struct(f"cmx_aerosol_activation_params_{sfx}",
                                           s("M_w", "R", "rho_w", "rho_i", "sigma", "g", "f1", "f2", "g1", "g2", "p1", "p2"))
    ns.aerosol_mode = _struct(f"cmx_aerosol_mode_{sfx}", s("r_dry", "stdev", "N", "hygroscopicity", "molar_mass_mix"))
    ns.aerosol_distribution = _struct(f"cmx_aerosol_distribution_{sfx}", [
        ("n_modes", C.c_int32), ("pad_", C.c_int32), ("modes", ns.aerosol_mode * CMX_ARG_MAX_MODES)])
    # ---- P3
    ns.p3_params = _struct(f"cmx_p3_params_{sfx}",
                           s("alpha_va", "beta_va", "gamma", "sigma", "slope_a", "slope_b", "slope_c", "mu_max", "mu_const",
                             "rho_i", "rho_l", "tau_wet", "T_freeze"))
    ns.chen2022_small_ice_vel = _struct(f"cmx_chen2022_small_ice_vel_{sfx}", [
        ("A", ft * 3), ("B", ft * 3), ("C", ft * 4), ("E", ft * 3), ("F", ft * 3), ("G", ft * 3), ("cutoff", ft)])
    ns.chen2022_large_ice_vel = _struct(f"cmx_chen2022_large_ice_vel_{sfx}", [
        ("A", ft * 3), ("B", ft * 3), ("C", ft * 3), ("E", ft * 3), ("F", ft * 3), ("G", ft * 3), ("H", ft * 3), ("cutoff", ft)])
    ns.chen2022_ice_vel = _struct(f"cmx_chen2022_ice_vel_{sfx}", [
        ("small_ice", ns.chen2022_small_ice_vel), ("large_ice", ns.chen2022_large_ice_vel)])
    ns.quadrature = _struct(f"cmx_quadrature_{sfx}", [
        ("n", C.c_int32), ("reserved", C.c_int32), ("node", ft * CMX_QUAD_MAX), ("weight", ft * CMX_QUAD_MAX)])
    # ---- P3 liquid–ice collisions, immersion / deposition nucleation, P3IceParams
    ns.parameters_0m = _struct(f"cmx_parameters_0m_{sfx}", s("tau_precip", "qc_0", "S_0"))
    ns.local_rime_density = _struct(f"cmx_local_rime_density_{sfx}", s("a", "b", "c", "rho_ice"))
    ns.rain_freezing = _struct(f"cmx_rain_freezing_{sfx}", s("het_a", "het_B"))
    ns.mohler2006 = _struct(f"cmx_mohler2006_{sfx}", s("S_i_max", "T_thr"))
    ns.mohler_dust = _struct(f"cmx_mohler_dust_{sfx}", s("S0_warm", "S0_cold", "a_warm", "a_cold"))
    ns.deposition_dust = _struct(f"cmx_deposition_dust_{sfx}", s("deposition_m", "deposition_c"))
    ns.h2so4_solution_params = _struct(f"cmx_h2so4_solution_params_{sfx}", s("T_max", "T_min", "w_2", "c1", "c2", "c3", "c4", "c5", "c6", "c7"))
    ns.morrison_milbrandt2014 = _struct(f"cmx_morrison_milbrandt2014_{sfx}", s("T_dep_thres", "c1", "c2", "T0", "het_a", "het_B"))
    # ---- aerosol nucleation (src/parameters/AerosolModalNucleation.jl; the reference spells the first H2S04)
    ns.h2so4_nucleation = _struct(f"cmx_h2so4_nucleation_{sfx}", s(
        "p_b_n", "p_b_i", "u_b_n", "u_b_i", "v_b_n", "v_b_i", "w_b_n", "w_b_i", "p_t_n", "p_t_i", "u_t_n", "u_t_i", "v_t_n", "v_t_i",
        "w_t_n", "w_t_i", "p_A_n", "p_A_i", "a_n", "a_i"))
    ns.organic_nucleation = _struct(f"cmx_organic_nucleation_{sfx}", s(
        "a_1", "a_2", "a_3", "a_4", "a_5", "Y_MTO3", "Y_MTOH", "k_MTO3", "k_MTOH", "exp_MTO3", "exp_MTOH"))
    ns.mixed_nucleation = _struct(f"cmx_mixed_nucleation_{sfx}", s("k_H2SO4org", "k_MTOH", "exp_MTOH"))
    ns.p3_ice_params = _struct(f"cmx_p3_ice_params_{sfx}", [
        ("scheme", ns.p3_params), ("vent", ns.ventilation), ("rho_rim_local", ns.local_rime_density),
        ("vel_rain", ns.chen2022_rain_vel), ("vel_ice", ns.chen2022_ice_vel), ("cloud_pdf", ns.cloud_pdf_sb2006),
        ("rain_pdf", ns.rain_pdf_sb2006), ("ice_nucleation", ns.frostenberg2023), ("rain_freezing", ns.rain_freezing),
        ("tau_act", ft), ("quad", ns.quadrature)])
    # ---- the parcel model (parcel/ParcelModel.jl:12-43)
    ns.parcel_params = _struct(f"cmx_parcel_params_{sfx}", [
        ("tps", ns.thermo), ("aps", ns.air_properties), ("aap", ns.aerosol_activation_params), ("homogeneous", ns.koop2000),
        ("deposition", ns.mohler2006), ("p3", ns.morrison_milbrandt2014), ("ip", ns.frostenberg2023), ("aerosol_abifm", ns.abifm_dust),
        ("aerosol_deposition", ns.deposition_dust), ("aerosol_mohler", ns.mohler_dust)] + s(
        "const_dt", "r_nuc", "A_aer", "aero_sigma_g", "aero_N", "aero_M", "aero_kappa", "grav", "rho_w", "rho_i", "tau_relax_liq", "tau_relax_ice"))
    return ns


F32 = _family(C.c_float, "f32")
F64 = _family(C.c_double, "f64")


def family(FT):
    """Struct family for a float type given as 'f32'/'f64', numpy dtype or torch dtype."""
    name = str(FT)
    if name in ("f32", "float32", "torch.float32", "<class 'numpy.float32'>") or FT is np.float32:
        return F32
    if name in ("f64", "float64", "torch.float64", "<class 'numpy.float64'>") or FT is np.float64 or FT is float:
        return F64
    raise TypeError(f"unsupported float type {FT!r}")
