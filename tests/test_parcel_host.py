"""The parcel model without a GPU (include/cmx.h §(13), cmx/parcel.py):

  * the sub-rates of the NumPy restatement tests/parcel_ref.py against the oracle binding, to 1e-12, so that the restatement does not grade itself;
  * the device point functions and their host folding (csrc/cmx_parcel.hpp) compiled by g++ (tests/native/parcel_host.cpp) against the restatement,
    in both float types, at the bounds of the GPU test;
  * closed forms (the dry adiabat, the water and number budgets) and the qualitative content of the reference's examples;
  * for every ensemble tests/test_parcel_gpu.py runs: the restatement stays finite and the gate mask leaves out at most 1 % — a badly chosen draw
    fails here and not on the card;
  * argument statuses of the four entries and the Python wrapper's errors.
"""
import ctypes as C
import itertools
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

import parcel_cases as PC
import parcel_ref as R
from parity import FLOOR
from cmx import _abi, _lib, parcel
from cmx import parameters as P

REPO = Path(__file__).resolve().parent.parent
NPT, RTOL = PC.NPT, PC.RTOL
CT = {"f32": C.c_float, "f64": C.c_double}


@pytest.fixture(scope="module")
def ob(oracle):
    return oracle


def _quiet(f, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", P.UnpinnedParameterWarning)
        return f(*a, **k)


# ---- the restatement's sub-rates against the oracle ------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def test_restatement_sub_rates_match_the_oracle(ob):
    F = np.float64
    fam = _abi.F64
    pp, prm = PC.build("f64", aerosol="dust", aerosol_act="AeroAct", aero_σ_g=2.3, r_nuc=5e-8)
    tps_c, tps = pp.c.tps, prm["tps"]
    T = np.linspace(205.0, 300.0, 97)
    assert _rel(R.psat_liquid(F, tps, T), [ob.psat_liquid(fam, tps_c, float(t)) for t in T]) < 1e-12
    assert _rel(R.psat_ice(F, tps, T), [ob.psat_ice(fam, tps_c, float(t)) for t in T]) < 1e-12
    e = np.linspace(1.0, 3000.0, 97)
    ice, eT = ob.water_activity(fam, tps_c, T, e)
    assert _rel(R.a_w_ice(F, tps, T), ice) < 1e-12 and _rel(R.a_w_eT(F, tps, e, T), eT) < 1e-12
    # ABIFM_J and the Koop linear rate through the fused oracle entry (J_het, J_hom with the linear flag), deposition_J on its own
    Tc = np.linspace(225.0, 260.0, 71)
    a_w = np.linspace(0.8, 1.02, 71)
    o = ob.ice_nucleation_rates(fam, tps_c, pp.c.aerosol_abifm, pp.c.homogeneous, _abi.CMX_ICENUC_HOM_LINEAR, Tc, a_w, np.full(71, 1e-6))
    d = a_w - R.a_w_ice(F, tps, Tc)
    assert np.max(np.abs(d - o["delta_a_w"])) < 1e-14
    assert _rel(R.activity_J(F, prm["aerosol_abifm"]["ABIFM_m"], prm["aerosol_abifm"]["ABIFM_c"], o["delta_a_w"], 4), o["J_het"]) < 1e-12
    assert _rel(R.activity_J(F, prm["homogeneous"]["linear_c2"], prm["homogeneous"]["linear_c1"], o["delta_a_w"], 6), o["J_hom"]) < 1e-12
    dd = np.linspace(0.0, 0.4, 41)
    assert _rel(R.activity_J(F, prm["aerosol_deposition"]["deposition_m"], prm["aerosol_deposition"]["deposition_c"], dd, 4),
                ob.deposition_J(fam, pp.c.aerosol_deposition, dd)) < 1e-12
    # Mohler-2006 activated fraction on both sides of T_thr (S_i < S_i_max: the oracle returns NaN beyond, the parcel model's own gate handles that)
    Si, Tm = np.linspace(1.0, 1.34, 35), np.where(np.arange(35) % 2 == 0, 215.0, 235.0)
    f, _ = ob.mohler2006_deposition(fam, pp.c.aerosol_mohler, pp.c.deposition, Si, Tm, np.zeros(35), np.zeros(35))
    assert np.max(np.abs(R.mohler_activated_fraction(F, prm["aerosol_mohler"], prm["deposition"], Si, Tm) - f)) < 1e-12
    for t in (228.0, 233.0, 250.0, 273.0, 273.15, 280.0):
        assert abs(float(R.P3_deposition_N_i(F, prm["p3"], np.array([t]))[0]) - ob.P3_deposition_N_i(fam, pp.c.p3, t)) <= 1e-12 * 1e5
        if t < 273.15:
            assert abs(float(R.INP_concentration_mean(F, prm["ip"], np.array([t]))[0]) - ob.INP_concentration_mean(fam, pp.c.ip, t)) < 1e-12 * 40
    # P3_het_N_i where the reference's 1 − exp(x) does not cancel (x ≈ −1e-3 … −1: rain-sized volumes at cold temperatures)
    for t, V in ((240.0, 1e-12), (235.0, 1e-12), (250.0, 1e-10)):
        got = float(R.P3_het_N_i(F, prm["p3"], np.array([t]), np.array([1e6]), np.array([V]), F(1.0))[0])
        want = ob.P3_het_N_i(fam, pp.c.p3, t, 1e6, V, 1.0)
        assert abs(got - want) <= 1e-12 * 1e6, (t, V, got, want)
    # critical supersaturation through the ARG entries: u = 2 log(Sm/S_max)/(3 √2 log σ) and S_max give Sm
    ad = fam.aerosol_distribution()
    ad.n_modes = 1
    ad.modes[0] = fam.aerosol_mode(r_dry=5e-8, stdev=2.3, N=1e8, hygroscopicity=prm["aero_kappa"], molar_mass_mix=prm["aero_M"])
    Ta, pa, wa, qa = np.linspace(250.0, 290.0, 9), np.full(9, 8e4), np.full(9, 0.5), np.full(9, 3e-3)
    S_max = ob.arg2000_activation(fam, pp.c.aap, ad, pp.c.aps, tps_c, Ta, pa, wa, qa)["S_max"]
    u = ob.arg2000_erf_argument(fam, pp.c.aap, ad, pp.c.aps, tps_c, Ta, pa, wa, qa)[0]
    Sm = S_max * np.exp(u * 3 * np.sqrt(2.0) * np.log(2.3) / 2)
    assert _rel(R.critical_supersaturation(F, prm["aap"], prm["aero_kappa"], 5e-8, Ta), Sm) < 1e-12 * 50     # exp of u·3.5: a few ulp amplified


# ---- the g++ build of the point functions ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    out = REPO / "tests" / "native" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libparcel_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(REPO / "tests" / "native" / "parcel_host.cpp")],
                   check=True)
    return C.CDLL(str(so))


def _arr(ft, cols):
    return (C.POINTER(CT[ft]) * len(cols))(*[c.ctypes.data_as(C.POINTER(CT[ft])) if c is not None else None for c in cols])


def host_tendencies(host, ft, pp, Y, w, coef=None):
    n = Y[0].size
    dY = [np.full(n, -7.0, dtype=NPT[ft]) for _ in range(9)]
    proc = [np.full(n, -7.0, dtype=NPT[ft]) for _ in range(6)]
    ck = [None] * 6 if coef is None else [coef.get(k) for k in R.COEFFICIENTS]
    st = getattr(host, f"parcel_tendencies_{ft}")(C.byref(pp.c), C.c_uint32(pp.flags), C.c_int64(n), _arr(ft, Y), w.ctypes.data_as(C.POINTER(CT[ft])),
                                                 _arr(ft, ck), _arr(ft, dY), _arr(ft, proc))
    assert st == 0
    return dY, proc


def host_run(host, ft, pp, Y, w, n_steps):
    n = Y[0].size
    out = [np.empty(n, dtype=NPT[ft]) for _ in range(9)]
    st = getattr(host, f"parcel_run_{ft}")(C.byref(pp.c), C.c_uint32(pp.flags), C.c_int64(n), C.c_int64(n_steps), _arr(ft, Y),
                                          w.ctypes.data_as(C.POINTER(CT[ft])), None, _arr(ft, out))
    assert st == 0
    return out


def compare_tendencies(ft, got_dY, got_proc, ref, what, report=None):
    """|x − ref| ≤ rtol·max(|ref|, Σ|terms|) outside the gate mask; NaN exactly where the restatement has NaN.  Returns the worst normalised error."""
    keep = ~ref["near_gate"]
    assert np.mean(~keep) <= PC.EXCLUDED_CAP, (what, float(np.mean(~keep)))
    worst = 0.0
    proc_scale = ref["proc_scale"]
    rows = [(R.STATE[j], got_dY[j], ref["dY"][j], ref["scale"][j]) for j in range(9)] + \
           [(k, got_proc[i], ref["proc"][k], proc_scale[k]) for i, k in enumerate(R.PROCESS)]
    for name, x, r, sc in rows:
        x, r = np.asarray(x, dtype=np.float64)[keep], np.asarray(r, dtype=np.float64)[keep]
        assert np.array_equal(np.isnan(x), np.isnan(r)), (what, name, int(np.sum(np.isnan(x) != np.isnan(r))))
        den = np.maximum(np.abs(r), FLOOR[ft]) if sc is None else np.maximum(np.maximum(np.abs(r), sc[keep]), FLOOR[ft])   # FLOOR: the float type's underflow
        ok = ~np.isnan(r)
        same_inf = np.isinf(r) & (x == r)
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.where(same_inf | ((x == 0) & (r == 0)), 0.0, np.abs(x - r) / den)
        e = float(np.max(err[ok])) if ok.any() else 0.0
        if report is not None:
            report[name] = e
        assert e <= RTOL[ft], (what, name, e)
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("combo", list(PC.TENDENCY_COMBOS))
def test_point_function_matches_the_restatement(host, ft, combo):
    cfg = PC.TENDENCY_COMBOS[combo]
    pp, prm = PC.build(ft, **cfg["kw"])
    cols, w, nan_at = PC.tendency_states(20_001, 11, cfg["T"], prm["tps"])
    Y, w = [c.astype(NPT[ft]) for c in cols], w.astype(NPT[ft])
    ref = R.rhs(np.float64, prm, PC.ref_options(cfg["kw"]), Y, w, margin=PC.MARGIN[ft])
    dY, proc = host_tendencies(host, ft, pp, Y, w)
    compare_tendencies(ft, dY, proc, ref, f"host {ft} {combo}")
    for j, i in nan_at.items():                     # the NaN rule: every output of that parcel, no other parcel
        assert all(np.isnan(a[i]) for a in dY + proc), (j, i)
    assert sum(int(np.isnan(a).sum()) for a in dY[:1]) == len(nan_at)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_host_run_follows_the_restatement(host, ft):
    """The Euler recurrence of the point functions against the restatement over 100 steps, on the scales of the GPU test."""
    case = "abifm_cond_dep_mono"
    pp, prm = PC.build(ft, **PC.RUN_CASES[case]["kw"])
    Y0, w = PC.run_ensemble(case, prm)
    Y, w = [c.astype(NPT[ft])[:512] for c in Y0], w.astype(NPT[ft])[:512]
    ref = R.run(np.float64, prm, PC.ref_options(PC.RUN_CASES[case]["kw"]), Y, w, 100, margin=PC.MARGIN[ft])
    got = host_run(host, ft, pp, Y, w, 100)
    err = PC.scaled_run_error(got, ref["final"], [y.astype(np.float64) for y in Y])[:, ~ref["near_gate"]]
    bound = RTOL["f64"] if ft == "f64" else None
    if ft == "f64":
        assert float(np.max(err)) <= bound, np.max(err, axis=1)
    else:      # Float32: four times the reference-only spread of this ensemble at 100 steps (tests/golden/parcel_f32_spread.json)
        spread = PC.load_spread()[case]["100"]
        for j, name in enumerate(R.STATE):
            assert float(np.max(err[j])) <= PC.SPREAD_FACTOR * spread[name], (name, float(np.max(err[j])), spread[name])


# ---- closed forms -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_dry_adiabat_with_every_option_none(host, ft):
    pp, prm = PC.build(ft)
    Y0, w = R.ensemble(256, 5, prm["tps"], prm["rho_w"], with_ice=True, with_aerosol=True)
    Y, w = [c.astype(NPT[ft]) for c in Y0], w.astype(NPT[ft])
    dY, proc = host_tendencies(host, ft, pp, Y, w)
    for j in range(3, 9):
        assert not dY[j].any()                       # q_vap, q_liq, q_ice, N_* do not move
    assert not any(p.any() for p in proc)
    qt = (Y[3] + Y[4] + Y[5]).astype(np.float64)
    t = prm["tps"]
    cp_m = t["cp_d"] + (t["cp_v"] - t["cp_d"]) * qt + (t["cp_l"] - t["cp_v"]) * Y[4] + (t["cp_i"] - t["cp_v"]) * Y[5]
    lapse = -prm["grav"] / cp_m * w.astype(np.float64)
    assert np.max(np.abs(dY[2] / lapse - 1)) <= 8 * np.finfo(NPT[ft]).eps
    out = host_run(host, ft, pp, Y, w, 50)           # T falls by g/cp_m·w·dt per step: 50 steps, each rounding T once (half an ulp of T)
    fall = out[2].astype(np.float64) - Y[2]
    assert np.max(np.abs(fall - 50 * lapse * prm["const_dt"])) <= 50 * np.finfo(NPT[ft]).eps * 260.0
    for j in range(3, 9):
        assert np.array_equal(out[j], Y[j])


_OPTION_VALUES = [R.SUPPORTED[k] for k in R.DEFAULT_OPTIONS]


def test_water_and_number_budgets_for_every_option_combination(host):
    """dq_vap + dq_liq + dq_ice = 0 and dN_aer + dN_liq + dN_ice = dN_liq_ce + dN_ice_ds for all 2·4·4·3·3·3·2·2 = 3456 combinations."""
    ft = "f64"
    cols, w, _ = PC.tendency_states(1200, 3, (233.0, 270.0), PC.build(ft)[1]["tps"])
    Y, w = [np.ascontiguousarray(c[:64]) for c in cols], np.ascontiguousarray(w[:64])      # (the NaN parcels of the draw come after these)
    assert not np.isnan(np.sum(Y, axis=0) + w).any()
    Ycl = [np.maximum(y, 0.0) for y in Y]
    n_combos = 0
    for values in itertools.product(*_OPTION_VALUES):
        kw = dict(zip(R.DEFAULT_OPTIONS, values))
        pp, _ = PC.build(ft, aerosol="dust", aero_σ_g=2.3, r_nuc=5e-8, Nₐ=2e4, **kw)
        dY, proc = host_tendencies(host, ft, pp, Y, w)
        n_combos += 1
        dq = dY[3] + dY[4] + dY[5]
        sq = np.abs(dY[3]) + np.abs(dY[4]) + np.abs(dY[5])
        assert np.all(np.abs(dq) <= 4e-16 * sq), kw
        # the two number sinks, recomputed from the process terms the entry reports
        ce, ds = proc[4], proc[5]
        with np.errstate(divide="ignore", invalid="ignore"):
            dNl_ce = np.where((ce < 0) & (Ycl[4] > 0) & (Ycl[4] < 1e-6), Ycl[7] * ce / Ycl[4], 0.0)
            dNi_ds = np.where((ds < 0) & (Ycl[5] > 0) & (Ycl[5] < 1e-6), Ycl[8] * ds / Ycl[5], 0.0)
        dN = dY[6] + dY[7] + dY[8]
        sN = np.abs(dY[6]) + np.abs(dY[7]) + np.abs(dY[8]) + np.abs(dNl_ce) + np.abs(dNi_ds)
        assert np.all(np.abs(dN - (dNl_ce + dNi_ds)) <= 1e-14 * sN), kw
    assert n_combos == 3456


# ---- the qualitative content of the reference's examples ---------------------------------------------------------------------------------------
def test_example_liquid_only(host):
    """parcel/Example_Liquid_only.jl: S_l overshoots saturation, then relaxes towards it; q_liq grows."""
    ft = "f64"
    pp, prm = PC.build(ft, condensation_growth="Condensation", const_dt=1.0)
    T, p, Nl, r0 = 285.2, 7.7e4, 200e6, 8e-6
    ql = Nl * 4 / 3 * np.pi * r0 ** 3 * prm["rho_w"] / 1.2
    Y0, _ = R.ensemble(1, 0, prm["tps"], prm["rho_w"])
    Y0[0][:], Y0[1][:], Y0[2][:], Y0[4][:], Y0[7][:] = 1.0, p, T, ql, Nl
    esl = R.psat_liquid(np.float64, prm["tps"], Y0[2])
    a = 1.0 * esl / p / prm["tps"]["R_v"]
    Y0[3][:] = a * prm["tps"]["R_d"] * (1 - ql) / (1 - a * (prm["tps"]["R_v"] - prm["tps"]["R_d"]))
    w = np.array([1.0])
    S, q = [], []
    Y = [y.copy() for y in Y0]
    for _ in range(300):
        Y = host_run(host, ft, pp, Y, w, 1)
        S.append(float(Y[0][0]))
        q.append(float(Y[4][0]))
    peak = int(np.argmax(S))
    assert S[peak] > 1.0 + 1e-4 and 0 < peak < len(S) - 1 and S[-1] < S[peak] and S[-1] > 1.0
    assert all(b > a_ for a_, b in zip(q, q[1:])) and q[-1] > ql


def test_example_immersion_freezing(host):
    """parcel/Example_Immersion_Freezing.jl (ABIFM on Illite, Condensation, Deposition, w = 0.4 m/s, 600 s from 251 K): the frozen fraction
    N_ice/(N_liq + N_ice) grows monotonically, and the Gamma size distribution freezes more than the Monodisperse one from equal q, N: its mean
    radius 2/λ is 0.69 of the monodisperse one, condensation is slower, the supersaturation and with it the water activity stay higher."""
    ft = "f64"
    frac = {}
    for dist in ("Monodisperse", "Gamma"):
        pp, prm = PC.build(ft, heterogeneous="ABIFM", condensation_growth="Condensation", deposition_growth="Deposition", aerosol="illite",
                           liq_size_distribution=dist, ice_size_distribution=dist, const_dt=1.0)
        tps = prm["tps"]
        Nl, r0, p0, T0, qv = 2000.0, 1e-6, 800e2, 251.0, 8.1e-4
        ql = Nl * 4 / 3 * np.pi * r0 ** 3 * prm["rho_w"] / 1.2
        R_a = tps["R_d"] * (1 + (tps["R_v"] / tps["R_d"] - 1) * (qv + ql) - tps["R_v"] / tps["R_d"] * ql)
        S = qv * p0 * tps["R_v"] / R_a / float(R.psat_liquid(np.float64, tps, np.array([T0]))[0])
        Y = [np.array([v]) for v in (S, p0, T0, qv, ql, 0.0, 0.0, Nl, 0.0)]
        w = np.array([0.4])
        series = []
        for _ in range(60):
            Y = host_run(host, ft, pp, Y, w, 10)
            series.append(float(Y[8][0] / (Y[7][0] + Y[8][0])))
        assert all(b >= a for a, b in zip(series, series[1:])) and series[-1] > 0
        frac[dist] = np.array(series)
    # both end fully frozen.  The parcel starts just below saturation (S_l = 0.9996), where the two runs differ by 1e-7; from the time freezing
    # matters (half a percent frozen) until it is complete the Gamma run is ahead
    partly = (frac["Monodisperse"] > 5e-3) & (frac["Monodisperse"] < 1 - 1e-6)
    assert partly.sum() >= 5, frac
    assert np.all(frac["Gamma"][partly] > frac["Monodisperse"][partly]), frac


# ---- the ensembles of the GPU test, vetted on the CPU --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(PC.RUN_CASES))
def test_gpu_ensembles_are_finite_and_mostly_away_from_gates(case):
    cfg = PC.RUN_CASES[case]
    _, prm = PC.build("f64", **cfg["kw"])
    Y0, w = PC.run_ensemble(case, prm)
    opt = PC.ref_options(cfg["kw"])
    r64 = R.run(np.float64, prm, opt, Y0, w, cfg["steps64"], save_every=PC.SAVE_EVERY, margin=PC.MARGIN["f64"])
    assert np.all(np.isfinite(r64["trajectory"]))
    assert np.mean(r64["near_gate"]) <= PC.EXCLUDED_CAP, float(np.mean(r64["near_gate"]))
    if not cfg["steps32"]:
        return
    # Float32: the inputs rounded to Float32; the Float64 restatement of THOSE inputs is the yardstick, the Float32 restatement must stay finite
    Y32 = [y.astype(np.float32) for y in Y0]
    w32 = w.astype(np.float32)
    m32 = R.run(np.float64, prm, opt, Y32, w32, cfg["steps32"], margin=PC.MARGIN["f32"])
    assert np.all(np.isfinite(np.stack(m32["final"])))
    assert np.mean(m32["near_gate"]) <= PC.EXCLUDED_CAP, float(np.mean(m32["near_gate"]))
    r32 = R.run(np.float32, prm, opt, Y32, w32, cfg["steps32"])
    assert np.all(np.isfinite(np.stack(r32["final"])))


def test_committed_spread_is_what_the_tool_generates():
    """tests/golden/parcel_f32_spread.json comes from tests/parcel_ref.py alone (tools/gen_parcel_spread.py); one case is regenerated here."""
    import sys
    sys.path.insert(0, str(REPO / "tools"))
    import gen_parcel_spread as G
    case = "none"
    fresh = G.spread_of(case, [PC.RUN_CASES[case]["steps32"]])
    committed = PC.load_spread()[case]
    for steps, row in fresh.items():
        for name, v in row.items():
            assert abs(v - committed[steps][name]) <= 1e-6 * max(v, 1e-30), (steps, name)


# ---- statuses and the wrapper's errors -----------------------------------------------------------------------------------------------------------
_UNSUPPORTED_FLAGS = [_abi.CMX_PARCEL_DEP_MOHLER_RATE, _abi.CMX_PARCEL_HET_FROSTENBERG_RANDOM, _abi.CMX_PARCEL_HET_FROSTENBERG_STOCHASTIC,
                      _abi.CMX_PARCEL_COND_NONEQ, _abi.CMX_PARCEL_DEPGROWTH_NONEQ, _abi.CMX_PARCEL_LIQ_MONODISPERSE_MIX,
                      _abi.CMX_PARCEL_PRESCRIBED_THERMODYNAMICS]


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_argument_statuses_without_gpu(ft):
    lib = _lib.lib()
    pp, _ = PC.build(ft)
    tend, run = getattr(lib, f"cmx_parcel_tendencies_{ft}"), getattr(lib, f"cmx_parcel_run_{ft}")
    BAD, UNS, OK = _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED, _abi.CMX_OK
    nine = (C.c_void_p * 9)(*[4096 + 64 * k for k in range(9)])
    nulls = (C.c_void_p * 9)()
    wp = C.c_void_p(8192)
    huge = 16 * 0x7fffffff + 1
    t = lambda flags, n, state=nine, w=wp, out=nine, p=pp: tend(C.byref(p.c) if p else None, flags, n, state, w, None, out, None, None)  # noqa: E731
    r = lambda flags, n, steps=10, every=0, state=nine, w=wp, out=nine, p=pp: run(C.byref(p.c) if p else None, flags, n, steps, every, state, w, None,  # noqa: E731
                                                                                 out, None, None)
    for f in (t, r):
        assert f(0, 8, p=None) == BAD                                    # no parameters
        assert f(0, -1) == BAD and f(0, huge) == UNS and f(0, 0) == OK   # the count rule
        assert f(0, 0, state=None, w=None, out=None) == OK               # n = 0 returns before the columns matter
        assert f(0, 8, state=None) == BAD and f(0, 8, w=None) == BAD and f(0, 8, state=nulls) == BAD
        for flag in _UNSUPPORTED_FLAGS:
            assert f(flag, 8) == UNS, hex(flag)
            assert f(flag, -1) == UNS                                    # the options are checked before the count
        assert f(1 << 30, 8) == BAD and f(6 << 8, 8) == BAD and f(3 << 12, 8) == BAD and f(5 << 4, 8) == BAD    # bits / values outside every field
    assert t(0, 8, out=None) == BAD and t(0, 8, out=nulls) == BAD        # tendencies: at least one output
    assert r(0, 8, out=None) == BAD and r(0, 8, out=nulls) == BAD        # run: all nine outputs
    assert r(0, 8, steps=-1) == BAD and r(0, 8, every=-1) == BAD


def test_python_wrapper_errors():
    for name, (message, table) in parcel._OPTIONS.items():
        with pytest.raises(ValueError, match=message):
            parcel.parcel_params("f64", **{name: "no such option"})
        for value, bits in table.items():
            if bits is None:
                with pytest.raises(NotImplementedError, match=f"{name} = '{value}'"):
                    parcel.parcel_params("f64", **{name: value})
    with pytest.raises(NotImplementedError, match="prescribed_thermodynamics"):
        parcel.parcel_params("f64", prescribed_thermodynamics=True)
    with pytest.raises(TypeError, match="Mohler-2006"):
        parcel.parcel_params("f64", deposition="MohlerAF")
    pp = _quiet(parcel.parcel_params, "f64", const_dt=0.4)
    cpu = [torch.ones(4, dtype=torch.float64)] * 9
    with pytest.raises(ValueError, match="no CPU path"):
        parcel.run_parcel(cpu, 0.0, 4.0, pp)
    with pytest.raises(ValueError, match="no CPU path"):
        parcel.parcel_tendencies(cpu, pp)
    with pytest.raises(TypeError, match="CUDA tensor"):
        parcel.parcel_tendencies([1.0] * 9, pp)
    with pytest.raises(ValueError, match="whole number"):
        parcel.run_parcel(cpu, 0.0, 1.0, pp)                            # 1.0 / 0.4 steps: refused before the columns are looked at
    with pytest.raises(ValueError, match="ten rows"):
        parcel.run_parcel(cpu[:5], 0.0, 4.0, pp)
    # the flags word of a combination, field by field
    pp = _quiet(parcel.parcel_params, "f32", aerosol_act="AeroAct", deposition="P3_dep", heterogeneous="Frostenberg_mean", homogeneous="ABHOM",
                condensation_growth="NonEq_Condensation_simple", deposition_growth="Deposition", liq_size_distribution="Gamma",
                ice_size_distribution="Gamma")
    assert pp.flags == (1 | (4 << 4) | (4 << 8) | (1 << 12) | (2 << 16) | (1 << 20) | (1 << 24) | (1 << 26))
    assert pp.c.r_nuc == np.float32(0.5 * 1.e-4 * 1e-6) and pp.c.A_aer == np.float32(1e-9) and pp.c.aero_N == 1e8 and pp.c.const_dt == 1.0
    assert pp.c.rho_i == np.float32(P.WaterProperties("f32").rho_i) and C.sizeof(pp.c) == 69 * 4
