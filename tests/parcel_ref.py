"""NumPy restatement of the reference's adiabatic parcel model — parcel/ParcelModel.jl, ParcelTendencies.jl, ParcelDistributions.jl, ParcelCommon.jl —
vectorised over parcels, the steps in a Python loop, the float type a parameter: np.float64 is the yardstick of tests/test_parcel_host.py and
tests/test_parcel_gpu.py, np.float32 is used only for the reference-only spread of tools/gen_parcel_spread.py.

Every expression is written in the reference's own arrangement (quotients as quotients, powers as powers, exp / log as they stand there), NOT in the
device's log2-domain one; the sub-rates are checked against the oracle binding in tests/test_parcel_host.py so that this file does not grade itself.
np.maximum / np.minimum propagate NaN like Julia's max / min, and a comparison with a NaN is false as in Julia's ifelse.

One deliberate difference, the library's NaN rule (include/cmx.h §(13)): with `nan_rule=True` (default) a parcel with a NaN among its nine state
values, w or a coefficient column has NaN in every output; the reference's arithmetic carries a NaN only to the tendencies that read it.

Options are the reference's strings (parcel_params, ParcelModel.jl:12-43); the ones the library does not build raise NotImplementedError here too.
"""
import math

import numpy as np
from scipy import special as _sp

STATE = ("S_l", "p_air", "T", "q_vap", "q_liq", "q_ice", "N_aer", "N_liq", "N_ice")
PROCESS = ("dN_liq_act", "dN_ice_dep", "dN_ice_imm", "dN_ice_hom", "dq_liq_ce", "dq_ice_ds")
COEFFICIENTS = ("deposition_m", "deposition_c", "ABIFM_m", "ABIFM_c", "linear_c1", "linear_c2")

DEFAULT_OPTIONS = dict(aerosol_act="None", deposition="None", heterogeneous="None", homogeneous="None", condensation_growth="None",
                       deposition_growth="None", liq_size_distribution="Monodisperse", ice_size_distribution="Monodisperse")
SUPPORTED = dict(aerosol_act=("None", "AeroAct"), deposition=("None", "MohlerAF", "ABDINM", "P3_dep"),
                 heterogeneous=("None", "ABIFM", "P3_het", "Frostenberg_mean"), homogeneous=("None", "ABHOM", "P3_hom"),
                 condensation_growth=("None", "Condensation", "NonEq_Condensation_simple"),
                 deposition_growth=("None", "Deposition", "NonEq_Deposition_simple"),
                 liq_size_distribution=("Monodisperse", "Gamma"), ice_size_distribution=("Monodisperse", "Gamma"))


def options(**kw):
    o = dict(DEFAULT_OPTIONS)
    for k, v in kw.items():
        if k not in o:
            raise KeyError(k)
        if v not in SUPPORTED[k]:
            raise NotImplementedError(f"{k} = {v!r}")
        o[k] = v
    return o


def parameters(struct):
    """Plain-float view of a cmx_parcel_params_* ctypes struct (cmx.parcel.parcel_params(...).c): {field: float | {field: float}}."""
    import ctypes as C
    out = {}
    for name, _ in struct._fields_:
        v = getattr(struct, name)
        out[name] = parameters(v) if isinstance(v, C.Structure) else float(v)
    return out


# ---- sub-rates (checked against the oracle binding in tests/test_parcel_host.py) -------------------------------------------------------------
def _sat(FT, tps, T, LH_0, cp_x):
    # TD.saturation_vapor_pressure: p_tr (T/T_tr)^(Δcp/R_v) exp((LH_0 − Δcp T_0)/R_v (1/T_tr − 1/T))
    dcp = FT(tps["cp_v"]) - FT(cp_x)
    R_v, T_0, T_tr = FT(tps["R_v"]), FT(tps["T_0"]), FT(tps["T_triple"])
    return FT(tps["press_triple"]) * (T / T_tr) ** (dcp / R_v) * np.exp((FT(LH_0) - dcp * T_0) / R_v * (FT(1) / T_tr - FT(1) / T))


def psat_liquid(FT, tps, T):
    return _sat(FT, tps, T, tps["LH_v0"], tps["cp_l"])


def psat_ice(FT, tps, T):
    return _sat(FT, tps, T, tps["LH_s0"], tps["cp_i"])


def a_w_eT(FT, tps, e, T):                       # Common.jl:250-253
    return e / psat_liquid(FT, tps, T)


def a_w_ice(FT, tps, T):                         # Common.jl:267-271
    return psat_ice(FT, tps, T) / psat_liquid(FT, tps, T)


def xi(FT, tps, T):                              # ParcelCommon.jl:4-6
    return psat_liquid(FT, tps, T) / psat_ice(FT, tps, T)


def activity_J(FT, m, c, delta_a_w, shift):      # ABIFM_J, deposition_J (shift 4), homogeneous_J_linear (shift 6; m = linear_c2, c = linear_c1)
    return FT(10) ** (m * delta_a_w + c + FT(shift))


def mohler_activated_fraction(FT, dust, ip, Si, T):      # IceNucleation.jl:44-53 (without the assertion)
    warm = T > FT(ip["T_thr"])
    S0 = np.where(warm, FT(dust["S0_warm"]), FT(dust["S0_cold"]))
    a = np.where(warm, FT(dust["a_warm"]), FT(dust["a_cold"]))
    return np.maximum(FT(0), np.exp(a * (Si - S0)) - FT(1))


def P3_deposition_N_i(FT, ip, T):                # IceNucleation.jl:162-166
    Tp = np.maximum(FT(ip["T_dep_thres"]), T)
    N = FT(1000) * FT(ip["c1"]) * np.exp(FT(ip["c2"]) * (FT(ip["T0"]) - Tp))
    return np.where(T < FT(ip["T0"]), N, FT(0))


def P3_het_N_i(FT, ip, T, N_l, V_l, dt):         # IceNucleation.jl:202-205
    # as −N_l·expm1(x), the form the library states for this function (include/cmx.h §(11), tests/nucleation_ref.py): the reference's
    # N_l (1 − exp(x)) cancels for the |x| ≪ 1 of cloud droplets (x ≈ 1e-13 at 260 K: a 1e-3 error even in Float64); both agree to rounding elsewhere
    Ts = FT(ip["T0"]) - T
    return -N_l * np.expm1(-FT(ip["het_B"]) * V_l * dt * np.exp(FT(ip["het_a"]) * Ts))


def INP_concentration_mean(FT, ip, T):           # IceNucleation.jl:250-253
    Tc = np.minimum(T - FT(ip["T_freeze"]), FT(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return FT(9) * np.log(-FT(ip["b"]) * Tc / FT(10)) - FT(ip["log_a"])


def coeff_of_curvature(FT, ap, T):               # AerosolActivation.jl:35-40
    return FT(2) * FT(ap["sigma"]) * FT(ap["M_w"]) / FT(ap["rho_w"]) / FT(ap["R"]) / T


def critical_supersaturation(FT, ap, kappa, r_dry, T):    # AerosolActivation.jl:107-118, one Mode_κ with one component
    A = coeff_of_curvature(FT, ap, T)
    return FT(2) / np.sqrt(FT(kappa)) * (A / FT(3) / FT(r_dry)) ** FT(3 / 2)


def G_func(FT, aps, tps, T, L, p_vs):            # Common.jl:47-102
    eps_1m = FT(np.cbrt(np.finfo(FT).tiny))
    p_safe = np.maximum(p_vs, eps_1m)
    D, K, R_v = np.maximum(FT(aps["D_vapor"]), eps_1m), np.maximum(FT(aps["K_therm"]), eps_1m), FT(tps["R_v"])
    return FT(1) / (L / K / T * (L / R_v / T - FT(1)) + R_v * T / D / p_safe)


def distribution_moments(FT, kind, q, N, rho, rho_air):   # ParcelDistributions.jl:11-23, 54-74: (r, V)
    pi = FT(np.pi)
    with np.errstate(all="ignore"):
        if kind == "Monodisperse":
            r = np.cbrt(q / N / FT(4 / 3 * np.pi) / rho * rho_air)
            V = FT(4 / 3 * np.pi) * r ** 3
        elif kind == "Gamma":
            lam = np.cbrt(FT(32) * pi * N / q * rho / rho_air)
            r = FT(2) / lam
            V = FT(4) / FT(3) * pi * FT(24) / lam ** 3
        else:
            raise NotImplementedError(kind)
    none = (N == 0) | (q == 0)
    return np.where(none, FT(0), r), np.where(none, FT(0), V)


# ---- the right-hand side ----------------------------------------------------------------------------------------------------------------------
def _near(x, x0, margin):
    return np.abs(x - x0) <= margin * np.maximum(np.abs(x0), np.abs(x))


def rhs(FT, prm, opt, Y, w, coefficients=None, margin=0.0, nan_rule=True):
    """parcel_model(dY, Y, p, t).  Y: nine arrays (STATE order), w: array.  coefficients: {name: array} overriding COEFFICIENTS per parcel.
    Returns dict(dY=[9 arrays], proc={PROCESS: array}, scale=[9 arrays] and proc_scale={PROCESS: array}: Σ|operand terms| of each output (the
    cancellation scale of SURVEY H3: a difference such as AF·Nₐ − Nᵢ, Sᵢ − 1 or N ½(1 − erf u) − (Nₐ⁰ − Nₐ) is accurate to the rounding of its
    operands, not of its value), near_gate=bool array)."""
    FT = np.dtype(FT).type
    f = FT
    Y = [np.asarray(y, dtype=FT) for y in Y]
    w = np.asarray(w, dtype=FT)
    tps, aps, ap = prm["tps"], prm["aps"], prm["aap"]
    coefficients = coefficients or {}
    k = {"deposition_m": prm["aerosol_deposition"]["deposition_m"], "deposition_c": prm["aerosol_deposition"]["deposition_c"],
         "ABIFM_m": prm["aerosol_abifm"]["ABIFM_m"], "ABIFM_c": prm["aerosol_abifm"]["ABIFM_c"],
         "linear_c1": prm["homogeneous"]["linear_c1"], "linear_c2": prm["homogeneous"]["linear_c2"]}
    k = {n: (np.asarray(coefficients[n], dtype=FT) if coefficients.get(n) is not None else f(v)) for n, v in k.items()}
    dt, r_nuc, eps = f(prm["const_dt"]), f(prm["r_nuc"]), np.finfo(FT).eps
    rho_l, rho_i, grav, R_v = f(prm["rho_w"]), f(prm["rho_i"]), f(prm["grav"]), f(tps["R_v"])
    pi = f(np.pi)
    near = np.zeros(Y[0].shape, dtype=bool)
    with np.errstate(all="ignore"):
        S, p, T = Y[0], Y[1], Y[2]
        qv, ql, qi, Na, Nl, Ni = [np.maximum(y, f(0)) for y in Y[3:9]]            # clip! of rows 4–9
        qt = qv + ql + qi
        R_d = f(tps["R_d"])
        R_air = R_d * (f(1) + (R_v / R_d - f(1)) * qt - R_v / R_d * (ql + qi))     # TD.gas_constant_air
        cp_air = f(tps["cp_d"]) + (f(tps["cp_v"]) - f(tps["cp_d"])) * qt + (f(tps["cp_l"]) - f(tps["cp_v"])) * ql \
            + (f(tps["cp_i"]) - f(tps["cp_v"])) * qi                                  # TD.cp_m
        T_0 = f(tps["T_0"])
        L_vap = f(tps["LH_v0"]) + (f(tps["cp_v"]) - f(tps["cp_l"])) * (T - T_0)
        L_subl = f(tps["LH_s0"]) + (f(tps["cp_v"]) - f(tps["cp_i"])) * (T - T_0)
        L_fus = (f(tps["LH_s0"]) - f(tps["LH_v0"])) + (f(tps["cp_l"]) - f(tps["cp_i"])) * (T - T_0)
        rho_air = p / (R_air * T)
        e = qv * p * R_v / R_air
        esl = psat_liquid(FT, tps, T)
        r_l, V_l = distribution_moments(FT, opt["liq_size_distribution"], ql, Nl, rho_l, rho_air)
        r_i, _ = distribution_moments(FT, opt["ice_size_distribution"], qi, Ni, rho_i, rho_air)
        zero = np.zeros_like(S)

        # aerosol activation
        dNl_act = s_act = zero
        if opt["aerosol_act"] == "AeroAct":
            smax = np.maximum(f(0), S - f(1))
            sm = critical_supersaturation(FT, ap, prm["aero_kappa"], r_nuc, T)
            u = f(2) * np.log(sm / smax) / f(3) / np.sqrt(f(2)) / np.log(f(prm["aero_sigma_g"]))
            erf_u = _sp.erf(u.astype(np.float64)).astype(FT)
            dNl_act = np.maximum(f(0), f(prm["aero_N"]) * f(1 / 2) * (f(1) - erf_u) - (f(prm["aero_N"]) - Na)) / f(1)
            s_act = f(prm["aero_N"]) * f(1 / 2) * (f(1) - erf_u) + np.abs(f(prm["aero_N"]) - Na)
            near |= _near(S - f(1), eps, margin) | _near(dNl_act, eps, margin)
        A = coeff_of_curvature(FT, ap, T)
        r_act = np.where((dNl_act < eps) | ((S - f(1)) < eps), r_nuc, np.minimum(f(1e-6), f(2 / 3) * A / (S - f(1))))
        dql_act = dNl_act * f(4) * pi / f(3) * r_act ** 3 * rho_l / rho_air
        s_qact = np.maximum(s_act, np.abs(dNl_act)) * f(4) * pi / f(3) * r_act ** 3 * rho_l / rho_air

        # deposition nucleation
        dNi_dep = zero
        s_dep = None
        if opt["deposition"] == "MohlerAF":
            Si = xi(FT, tps, T) * S
            S_max = f(prm["deposition"]["S_i_max"])
            AF = np.where(Si >= S_max, f(0), mohler_activated_fraction(FT, prm["aerosol_mohler"], prm["deposition"], Si, T))
            dNi_dep = np.maximum(f(0), AF * Na - Ni) / dt
            s_dep = ((AF + f(2)) * Na + Ni) / dt                     # AF = exp(…) − 1: the operands are exp(…), 1 and Nᵢ
            near |= _near(Si, S_max, margin) | _near(T, f(prm["deposition"]["T_thr"]), margin)
        elif opt["deposition"] == "ABDINM":
            d_aw = a_w_eT(FT, tps, e, T) - a_w_ice(FT, tps, T)
            J = activity_J(FT, k["deposition_m"], k["deposition_c"], d_aw, 4)
            dNi_dep = np.minimum(J * Na * (f(4) * pi * r_nuc ** 2), Na / dt)
        elif opt["deposition"] == "P3_dep":
            N_dep = P3_deposition_N_i(FT, prm["p3"], T)
            dNi_dep = np.minimum(np.maximum(f(0), (N_dep - Ni) / dt), Na / dt)
            s_dep = (N_dep + Ni) / dt
            near |= _near(T, f(prm["p3"]["T0"]), margin)
        elif opt["deposition"] != "None":
            raise NotImplementedError(opt["deposition"])
        dqi_dep = dNi_dep * f(4) / f(3) * pi * r_nuc ** 3 * rho_i / rho_air
        s_dep = np.abs(dNi_dep) if s_dep is None else np.maximum(s_dep, np.abs(dNi_dep))
        s_qdep = s_dep * f(4) / f(3) * pi * r_nuc ** 3 * rho_i / rho_air

        # heterogeneous ice nucleation
        dNi_imm = zero
        s_imm = None
        if opt["heterogeneous"] == "ABIFM":
            d_aw = a_w_eT(FT, tps, e, T) - a_w_ice(FT, tps, T)
            J = activity_J(FT, k["ABIFM_m"], k["ABIFM_c"], d_aw, 4)
            dNi_imm = np.minimum(J * Nl * f(prm["A_aer"]), Nl / dt)
        elif opt["heterogeneous"] == "P3_het":
            N_het = P3_het_N_i(FT, prm["p3"], T, Nl, V_l, dt)
            dNi_imm = np.minimum(np.maximum(f(0), (N_het - Ni) / dt), Nl / dt)
            s_imm = (N_het + Ni) / dt
        elif opt["heterogeneous"] == "Frostenberg_mean":
            INPC = np.exp(INP_concentration_mean(FT, prm["ip"], T))
            dNi_imm = np.minimum(Nl, np.maximum(f(0), INPC - Ni)) / dt
            s_imm = (INPC + Ni) / dt
            near |= _near(T, f(prm["ip"]["T_freeze"]), margin)
        elif opt["heterogeneous"] != "None":
            raise NotImplementedError(opt["heterogeneous"])
        dqi_imm = dNi_imm * V_l * rho_i / rho_air
        s_imm = np.abs(dNi_imm) if s_imm is None else np.maximum(s_imm, np.abs(dNi_imm))
        s_qimm = s_imm * V_l * rho_i / rho_air

        # homogeneous ice nucleation
        dNi_hom = zero
        if opt["homogeneous"] == "ABHOM":
            e_h = esl * S
            d_aw = a_w_eT(FT, tps, e_h, T) - a_w_ice(FT, tps, T)
            J = activity_J(FT, k["linear_c2"], k["linear_c1"], d_aw, 6)
            dNi_hom = np.minimum(J * Nl * V_l, Nl / dt)
        elif opt["homogeneous"] == "P3_hom":
            dNi_hom = np.where((T < f(233.15)) & (Nl > f(0)), Nl / dt, f(0))
            near |= _near(T, f(233.15), margin)
        elif opt["homogeneous"] != "None":
            raise NotImplementedError(opt["homogeneous"])
        dqi_hom = dNi_hom * V_l * rho_i / rho_air

        # condensation / evaporation
        def limited(dq, q_cond):
            return np.where(dq > f(0), np.minimum(dq, qv / dt / 1), -np.minimum(np.abs(dq), q_cond / dt / 1))
        dql_ce = zero
        s_ce = None
        if opt["condensation_growth"] == "Condensation":
            G_l = G_func(FT, aps, tps, T, L_vap, esl)
            dql_ce = limited(f(4) * pi / rho_air * (S - f(1)) * G_l * r_l * Nl, ql)
        elif opt["condensation_growth"] == "NonEq_Condensation_simple":
            dql_ce = (np.maximum(S * qv - qv, f(0)) - ql) / f(prm["tau_relax_liq"])
            s_ce = (np.abs(S * qv) + qv + ql) / f(prm["tau_relax_liq"])
        elif opt["condensation_growth"] != "None":
            raise NotImplementedError(opt["condensation_growth"])
        s_ce = np.abs(dql_ce) if s_ce is None else np.maximum(s_ce, np.abs(dql_ce))
        dNl_ce = np.where((dql_ce < f(0)) & (ql > f(0)) & (ql < f(1e-6)), Nl * dql_ce / ql, f(0))
        near |= (dql_ce < f(0)) & _near(ql, f(1e-6), margin)
        # deposition / sublimation
        dqi_ds = zero
        s_ds = None
        if opt["deposition_growth"] == "Deposition":
            Si = xi(FT, tps, T) * S
            G_i = G_func(FT, aps, tps, T, L_subl, psat_ice(FT, tps, T))
            dqi_ds = limited(f(4) * pi / rho_air * (Si - f(1)) * G_i * r_i * Ni, qi)
            s_ds = np.abs(f(4) * pi / rho_air * (np.abs(Si) + f(1)) * G_i * r_i * Ni)      # Sᵢ − 1: the operands are ξ Sₗ and 1
        elif opt["deposition_growth"] == "NonEq_Deposition_simple":
            Si = xi(FT, tps, T) * S
            dqi_ds = (np.maximum(Si * qv - qv, f(0)) - qi) / f(prm["tau_relax_ice"])
            s_ds = (np.abs(Si * qv) + qv + qi) / f(prm["tau_relax_ice"])
        elif opt["deposition_growth"] != "None":
            raise NotImplementedError(opt["deposition_growth"])
        s_ds = np.abs(dqi_ds) if s_ds is None else np.maximum(s_ds, np.abs(dqi_ds))
        dNi_ds = np.where((dqi_ds < f(0)) & (qi > f(0)) & (qi < f(1e-6)), Ni * dqi_ds / qi, f(0))
        near |= (dqi_ds < f(0)) & _near(qi, f(1e-6), margin)

        dNi = dNi_dep + dNi_imm + dNi_hom + dNi_ds
        dNa = -dNi_dep - dNl_act
        dNl = dNl_act - dNi_imm - dNi_hom + dNl_ce
        dql_v2l = dql_ce + dql_act
        dqi_l2i = dqi_imm + dqi_hom
        dqi_v2i = dqi_dep + dqi_ds
        dqi = dqi_v2i + dqi_l2i
        dql = dql_v2l - dqi_l2i
        dqv = -dql_v2l - dqi_v2i
        dp = -p * grav / R_air / T * w
        tT = [-grav / cp_air * w, L_vap / cp_air * dql_v2l, L_fus / cp_air * dqi_l2i, L_subl / cp_air * dqi_v2i]
        dT = tT[0] + tT[1] + tT[2] + tT[3]
        de_1, de_2 = dqv * p * R_v / R_air, qv * dp * R_v / R_air
        de = de_1 + de_2
        desl = L_vap * esl / R_v / T ** 2 * dT
        tS = [f(1) / esl * de, e / esl ** 2 * desl]
        dS = tS[0] - tS[1]
        # Σ|terms| for the cancellation rule: every tendency is a sum of terms of both signs — dT of four, dS of the two de terms and
        # the four dT terms through desl, the budgets of their process terms
        s_v2l, s_l2i, s_v2i = s_ce + s_qact, s_qimm + np.abs(dqi_hom), s_qdep + s_ds
        scale_T = np.abs(tT[0]) + np.abs(L_vap / cp_air) * s_v2l + np.abs(L_fus / cp_air) * s_l2i + np.abs(L_subl / cp_air) * s_v2i
        scale_S = ((s_v2l + s_v2i) * np.abs(p * R_v / R_air) + np.abs(de_2)) / esl + e / esl ** 2 * np.abs(L_vap * esl / R_v / T ** 2) * scale_T
        ab = np.abs
        s_act = np.maximum(s_act, ab(dNl_act))
        s_Nce = np.where(dNl_ce != 0, Nl * s_ce / ql, f(0))           # the number sinks carry the relative error of their growth term
        s_Nds = np.where(dNi_ds != 0, Ni * s_ds / qi, f(0))
        scales = [scale_S, ab(dp), scale_T, s_v2l + s_v2i, s_v2l + s_l2i, s_v2i + s_l2i, s_dep + s_act, s_act + s_imm + ab(dNi_hom) + s_Nce,
                  s_dep + s_imm + ab(dNi_hom) + s_Nds]
        proc_scales = [s_act, s_dep, s_imm, ab(dNi_hom), s_ce, s_ds]
    dY = [np.broadcast_to(np.asarray(d, dtype=FT), S.shape).copy() for d in (dS, dp, dT, dqv, dql, dqi, dNa, dNl, dNi)]
    proc = {n: np.broadcast_to(np.asarray(v, dtype=FT), S.shape).copy()
            for n, v in zip(PROCESS, (dNl_act, dNi_dep, dNi_imm, dNi_hom, dql_ce, dqi_ds))}
    if nan_rule:
        bad = np.isnan(w)
        for y in Y:
            bad = bad | np.isnan(y)
        for v in k.values():
            bad = bad | np.isnan(v)
        for a in dY + list(proc.values()):
            a[bad] = np.nan
    scale = [np.broadcast_to(np.asarray(v, dtype=np.float64), S.shape) for v in scales]
    proc_scale = {n: np.broadcast_to(np.asarray(v, dtype=np.float64), S.shape) for n, v in zip(PROCESS, proc_scales)}
    return dict(dY=dY, proc=proc, scale=scale, proc_scale=proc_scale, near_gate=near)


def run(FT, prm, opt, Y0, w, n_steps, save_every=0, coefficients=None, margin=0.0, nan_rule=True):
    """run_parcel: n_steps steps of ODE.Euler with dt = const_dt.  Returns dict(final=[9 arrays], trajectory=[record][9][n] array or None,
    near_gate=bool array: the parcel came within `margin` (relative) of a discontinuous gate at some step)."""
    FT = np.dtype(FT).type
    Y = [np.array(y, dtype=FT) for y in Y0]
    w = np.asarray(w, dtype=FT)
    dt = FT(prm["const_dt"])
    if nan_rule:
        bad = np.isnan(w)
        for y in Y:
            bad = bad | np.isnan(y)
        for y in Y:
            y[bad] = np.nan
    near = np.zeros(Y[0].shape, dtype=bool)
    traj = [np.stack(Y)] if save_every else None
    for s in range(1, n_steps + 1):
        r = rhs(FT, prm, opt, Y, w, coefficients, margin, nan_rule)
        near |= r["near_gate"]
        Y = [(y + dt * d).astype(FT) for y, d in zip(Y, r["dY"])]
        if save_every and s % save_every == 0:
            traj.append(np.stack(Y))
    return dict(final=Y, trajectory=np.stack(traj) if save_every else None, near_gate=near)


# ---- the ensembles of the tests ---------------------------------------------------------------------------------------------------------------
def ensemble(n, seed, tps, rho_w, with_ice=False, with_aerosol=False, cold=False):
    """Initial states in Float64 and w: T₀ ~ U(243, 258) (U(228, 240) if `cold`), p₀ ~ U(6e4, 9e4), w ~ U(0.1, 2), N_liq ~ U(500, 5000) droplets of
    r₀ = 1 µm, S_l ~ U(0.95, 1.02); optionally N_ice ~ U(1, 100) crystals of 1 µm and N_aer ~ U(1e3, 1e4)."""
    rng = np.random.default_rng(seed)
    T = rng.uniform(228.0, 240.0, n) if cold else rng.uniform(243.0, 258.0, n)
    p = rng.uniform(6e4, 9e4, n)
    w = rng.uniform(0.1, 2.0, n)
    Nl = rng.uniform(500.0, 5000.0, n)
    S = rng.uniform(0.95, 1.02, n)
    r0 = 1e-6
    ql = Nl * 4 / 3 * math.pi * r0 ** 3 * rho_w / 1.2
    Ni = rng.uniform(1.0, 100.0, n) if with_ice else np.zeros(n)
    qi = Ni * 4 / 3 * math.pi * r0 ** 3 * 916.7 / 1.2
    Na = rng.uniform(1e3, 1e4, n) if with_aerosol else np.zeros(n)
    esl = psat_liquid(np.float64, tps, T)
    # q_vap from S_l = q_v p R_v/R_air/e_sl with R_air = R_d (1 + (R_v/R_d − 1) q_t − R_v/R_d (q_l + q_i)): linear in q_v
    R_v, R_d = tps["R_v"], tps["R_d"]
    a = S * esl / p / R_v                                  # q_v / R_air
    qv = a * R_d * (1 - (ql + qi)) / (1 - a * (R_v - R_d))
    return [S, p, T, qv, ql, qi, Na, Nl, Ni], w
