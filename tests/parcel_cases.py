"""The option combinations, ensembles and bounds shared by tests/test_parcel_host.py, tests/test_parcel_gpu.py and tools/gen_parcel_spread.py, so that
the CPU suite vets (finite, exclusion share under the cap) exactly the ensembles the GPU suite runs, and the Float32 bound is generated for them."""
import json
import warnings
from pathlib import Path

import numpy as np

import parcel_ref as R

REPO = Path(__file__).resolve().parent.parent
SPREAD_FILE = REPO / "tests" / "golden" / "parcel_f32_spread.json"

RTOL = {"f32": 1e-3, "f64": 1e-6}                      # the project's plain bounds (tests/parity.py)
NPT = {"f32": np.float32, "f64": np.float64}
# relative margin of the gate mask (parcel_ref.rhs `near_gate`): well above the rounding of the float type that is compared, so that a parcel outside
# the margin takes the same side of every discontinuous gate in both computations
MARGIN = {"f32": 1e-4, "f64": 1e-9}
EXCLUDED_CAP = 0.01                                    # at most 1 % of an ensemble may be left out by the gate mask
SPREAD_FACTOR = 4.0                                    # Float32 run bound = 4 × the reference-only Float32-vs-Float64 spread (tools/gen_parcel_spread.py)


def build(ft, **kw):
    """cmx.parcel.parcel_params and its plain-float view for the restatement."""
    from cmx import parameters as P
    from cmx import parcel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", P.UnpinnedParameterWarning)
        aer = kw.pop("aerosol", None)
        if aer == "illite":
            aer = parcel.Aerosol(abifm=P.Illite(ft))
        elif aer == "dust":        # a dust with all three coefficient sets and, for AeroAct, sulfate's M and κ
            s = P.Sulfate(ft)
            aer = parcel.Aerosol(abifm=P.Illite(ft), deposition=P.DepositionDust(ft, "Kaolinite"), mohler=P.DesertDust(ft), M=s.M, kappa=s.kappa)
        pp = parcel.parcel_params(ft, aerosol=aer, **kw)
    return pp, R.parameters(pp.c)


def ref_options(kw):
    return R.options(**{k: v for k, v in kw.items() if k in R.DEFAULT_OPTIONS})


# ---- parcel_tendencies: every supported option value appears in at least one combination -------------------------------------------------------
TENDENCY_COMBOS = {
    "none": dict(kw=dict(), T=(225.0, 280.0)),
    "act_mohler_abifm_p3hom_cond_dep": dict(
        kw=dict(aerosol_act="AeroAct", deposition="MohlerAF", heterogeneous="ABIFM", homogeneous="P3_hom", condensation_growth="Condensation",
                deposition_growth="Deposition", aerosol="dust", aero_σ_g=2.3, r_nuc=5e-8, Nₐ=2e4), T=(212.0, 275.0)),
    # ABHOM: T ≥ 238 K keeps J_hom·N_liq inside the Float32 range for S_l ≤ 1.06 and N_liq ≤ 3e8 (J_hom = 10^(256 Δa_w − 62.5) is 1e34 m⁻³ s⁻¹ at
    # 225 K and S_l = 1; beyond the range Float32 gives Inf·0 = NaN for an absent droplet volume, in the reference's Float32 arithmetic as here)
    "abdinm_p3het_abhom_noneq_gamma": dict(
        kw=dict(deposition="ABDINM", heterogeneous="P3_het", homogeneous="ABHOM", condensation_growth="NonEq_Condensation_simple",
                deposition_growth="NonEq_Deposition_simple", liq_size_distribution="Gamma", ice_size_distribution="Gamma", aerosol="dust"),
        T=(238.0, 275.0)),
    "p3dep_frostenberg_gamma_liq": dict(kw=dict(deposition="P3_dep", heterogeneous="Frostenberg_mean", liq_size_distribution="Gamma"), T=(225.0, 280.0)),
}
N_TENDENCY = 200_001                                   # odd, ≥ 2e5


def tendency_states(n, seed, T_range, tps):
    """Broad random states: zeros, negatives (the clip), contents on both sides of 1e-6, a few NaN.  q_vap is the one that makes the vapour pressure
    S_l·e_sl(T) (to within the condensate's share of R_air), so that the two water activities the schemes form, e/e_sl and S_l, are the same physical
    state and the activity-based rates stay inside the Float32 range.  Float64 arrays; the tests round them to the float type."""
    rng = np.random.default_rng(seed)
    u = rng.uniform
    S, p, T, w = u(0.9, 1.06, n), u(2e4, 1e5, n), u(*T_range, n), u(-1.0, 5.0, n)
    ql, qi = 10.0 ** u(-9, -3.5, n), 10.0 ** u(-9, -3.5, n)
    Na, Nl, Ni = 10.0 ** u(0, 8, n), 10.0 ** u(0, 8.5, n), 10.0 ** u(-1, 6, n)
    a = S * R.psat_liquid(np.float64, tps, T) / p / tps["R_v"]
    qv = a * tps["R_d"] / (1 - a * (tps["R_v"] - tps["R_d"]))
    cols = [S, p, T, qv, ql, qi, Na, Nl, Ni]
    for c in cols[4:]:                                 # absent species and slightly negative values (the clip of rows 4–9)
        k = rng.random(n)
        c[k < 0.04] = 0.0
        c[(k >= 0.04) & (k < 0.05)] *= -1e-3
    nan_at = {}
    for j in range(10):                                # one NaN per input column, each in a parcel of its own
        i = 1000 + 17 * j
        (cols + [w])[j][i] = np.nan
        nan_at[j] = i
    return cols, w, nan_at


# ---- parcel_run: the ensembles of the issue (4096 draws, dt = 1 s) ---------------------------------------------------------------------------------
N_RUN = 4096
RUN_CASES = {
    # name: options, steps for the Float64 comparison, steps for the Float32 one (limited to where the Float32 restatement stays finite), ensemble
    "abifm_cond_dep_mono": dict(kw=dict(heterogeneous="ABIFM", condensation_growth="Condensation", deposition_growth="Deposition", aerosol="illite"),
                                steps64=600, steps32=200, ens=dict(seed=1)),
    "abifm_cond_dep_gamma": dict(kw=dict(heterogeneous="ABIFM", condensation_growth="Condensation", deposition_growth="Deposition", aerosol="illite",
                                         liq_size_distribution="Gamma", ice_size_distribution="Gamma"),
                                 steps64=600, steps32=200, ens=dict(seed=1)),
    "none": dict(kw=dict(), steps64=600, steps32=200, ens=dict(seed=2)),
    "p3dep_frostenberg_noneq": dict(kw=dict(deposition="P3_dep", heterogeneous="Frostenberg_mean", condensation_growth="NonEq_Condensation_simple",
                                            deposition_growth="NonEq_Deposition_simple"),
                                    steps64=300, steps32=None, ens=dict(seed=3, with_ice=True, with_aerosol=True)),
}
# steps32 = None: no Float32 run comparison.  In that ensemble q_liq relaxes to zero with τ = 10 s (S_l < 1 for most draws): after 100 steps it is
# 1e-16 kg/kg, 1e-13 of q_tot, and "four times the Float32-vs-Float64 spread of the restatement" would compare two rounding noises; the Float32 run test
# uses the ensembles whose spread the recurrence itself produces (the two ABIFM ones of the issue, and the dry adiabat).
F32_RUN_CASES = [k for k, v in RUN_CASES.items() if v["steps32"]]
SAVE_EVERY = 50


def run_ensemble(case, prm):
    return R.ensemble(N_RUN, tps=prm["tps"], rho_w=prm["rho_w"], **RUN_CASES[case]["ens"])


def run_scales(Y0):
    """The scale of each of the nine variables for the run comparison: S_l, p, T on their own magnitude (passed as None), the three q on the parcel's
    q_tot, the three N on its N_aer + N_liq + N_ice — the conserved totals of the initial state."""
    q_tot = Y0[3] + Y0[4] + Y0[5]
    N_tot = Y0[6] + Y0[7] + Y0[8]
    return [None, None, None, q_tot, q_tot, q_tot, N_tot, N_tot, N_tot]


def scaled_run_error(x, ref, Y0):
    """max over parcels of |x − ref| / scale per variable: [9] array (rows of x, ref: the nine variables)."""
    out = []
    for j, sc in enumerate(run_scales(Y0)):
        den = np.abs(np.asarray(ref[j], dtype=np.float64)) if sc is None else np.asarray(sc, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.abs(np.asarray(x[j], dtype=np.float64) - np.asarray(ref[j], dtype=np.float64)) / den)
    return np.stack(out)


def load_spread():
    return json.loads(SPREAD_FILE.read_text())
