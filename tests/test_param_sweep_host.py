"""The parameter sweep on the CPU (tests/param_sweep.py): every parameter a family's constructors read, changed one at a time.

* liveness — on the ORACLE ALONE, for every family and both float types: the reference must move at ≥ 50 states in the best entry of the family, or the
  parameter has a row in param_sweep.INERT.  This is what makes tests/test_param_sweep_gpu.py able to fail: it runs the same entries on the same states.
* parity — the device point functions compiled for the host (tests/native/point_host.cpp: host_sb2006, host_mp1m_tendencies, host_mp1m_sources,
  host_mp1m_linearized, host_sedimentation) against the oracle with the same override, at parity.RTOL / CTOL with the default knobs: the folded constants of
  make_sb_consts / make_mp1m_consts / make_vel1m_consts and the selection of the fast instantiations (return code of the harness), without a GPU.
* the Chen-2022 fit boundary and the aR ≥ bR domain, host twins of the device tests."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import param_sweep as S
import parity
from cmx import _abi
from cmx import parameters as P

REPO = Path(__file__).resolve().parent.parent
FAMILIES = ["SB2006", "1-moment", "0-moment", "cloud diagnostics", "ice nucleation", "ARG2000", "P3", "aerosol nucleation"]


@pytest.fixture(scope="module")
def host():
    out = REPO / "tests" / "native" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libparam_sweep_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(REPO / "tests" / "native" / "point_host.cpp")], check=True)
    return C.CDLL(str(so))


# liveness of every (entry, perturbation), shared by the tests below: {(family, ft): {parameter name: best count over entries and directions}}
_BEST, _NEAR = {}, {}


def _note(entry, ft, live):
    best = _BEST.setdefault((entry.family, ft), {})
    for n in entry.read():
        best.setdefault(n, 0)
    for key, v in live.items():
        n = key.split(" ")[0].split("[")[0]
        best[n] = max(best.get(n, 0), v)


def test_domain_pairs_stay_ordered():
    """× 1.25 of the lower member and × 0.8 of the upper one keep every ordered pair of the schemes ordered (limiters, xr_min < xr_max, Dr_th < Deq, xc_min < x*,
    Koop's Δa_w window, the H2SO4 fit range): no DOMAIN row is needed for them.  The rows that ARE needed name a parameter and a direction that exist."""
    d = P.DEFAULT_PARAMETERS
    for lo, hi in S.ORDERED_PAIRS:
        assert d[lo] * S.UP < d[hi] and d[lo] < d[hi] * S.DOWN, (lo, hi)
    assert d["SB2006_raindrops_terminal_velocity_coeff_aR"] * S.UP >= d["SB2006_raindrops_terminal_velocity_coeff_bR"]       # why the aR / bR rows exist
    assert d["latent_heat_vaporization_at_reference"] * S.UP > d["latent_heat_sublimation_at_reference"]
    for r in S.DOMAIN:
        assert r.name.split("[")[0] in d and r.label in ("x1.25", "x0.8") and r.reason
    # the P3 ventilation-factor rows are the perturbations at which the REFERENCE fails (NaN from the oracle where the default run is finite), no more, no fewer
    e = S.P3Melt()
    x64 = e.states("f64")[1]
    ref0 = e.ref(e.params(P.ParamDict("f64")), x64, "f64")
    cases, skipped = S.perturbations(e.read(), e.context)
    fails = lambda c: bool(np.any(np.isnan(e.ref(e.params(P.ParamDict("f64", c.override)), x64, "f64")["dLdt"]) & np.isfinite(ref0["dLdt"])))  # noqa: E731
    assert [c.key for c in skipped if c.name.startswith("Chen2022_table_B3") and not fails(c)] == []
    assert [c.key for c in cases if fails(c)] == []


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("k", range(len(S.all_entries())), ids=[str(e).replace(" ", "_") for e in S.all_entries()])
def test_entry(host, oracle, ft, k):
    """One entry: liveness of every perturbation on the oracle, and — where the device point function has a host build — its parity with the oracle."""
    e = S.all_entries()[k]
    rcs = {}

    def runner(p, x):
        rc, y = e.host(host, p, x, ft)
        rcs[rc] = rcs.get(rc, 0) + 1
        if rc < 0:
            raise RuntimeError(f"the host harness returned {rc}")
        return y
    sweep, live, skipped = S.run_sweep(e, ft, runner if e.host is not None else None)
    _note(e, ft, live)
    for s_ in skipped:
        print(f"[domain] {e} {ft}: {s_.key} skipped")
    if e.host is not None:
        print(f"[instantiations] {e} {ft}: harness return codes {rcs}")
        if isinstance(e, (S.SbTendencies, S.Mp1mTendencies)) and getattr(e, "optset", "default") == "default" and not isinstance(e, S.Mp1mLinearized):
            # the default options with a NON-exponent parameter changed run the fast instantiation (bit 0), an exponent the general one
            assert rcs.get(1, 0) + rcs.get(3, 0) > 100 and rcs.get(0, 0) + rcs.get(2, 0) >= 6, rcs
    sweep.finish()


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_every_parameter_is_seen_or_named_inert(oracle, ft):
    """Conditions (a) and (c): per family, every name the recorder saw moves the reference at ≥ 50 states in its best entry, or has a row in INERT (Float32 only:
    or in WEAK_F32, whose rows must then be seen in Float64); and INERT
    holds no row for a parameter that IS seen (a stale row would hide a later loss of coverage).  Runs after test_entry (same module): the counts are shared."""
    for fam in FAMILIES:
        ents = [e for e in S.all_entries() if e.family == fam]
        if (fam, ft) not in _BEST or any(n not in _BEST[(fam, ft)] for e in ents for n in e.read()):      # run alone (-k): measure here
            for e in ents:
                _note(e, ft, S.run_sweep(e, ft, None)[1])
        best, inert = _BEST[(fam, ft)], S.INERT[fam]
        weak_f32 = S.WEAK_F32.get(fam, {}) if ft == "f32" else {}
        weak = {n: v for n, v in best.items() if v < S.MIN_LIVE and n not in inert and n not in weak_f32}
        stale = [n for n in inert if best.get(n, 0) >= S.MIN_LIVE]
        swept = {n: v for n, v in best.items() if n not in inert and n not in weak_f32}
        print(f"\n[parameter sweep] {fam} {ft}: {len(swept)} parameters swept, smallest liveness {min(swept.values())} ({min(swept, key=swept.get)}); "
              f"inert: {sorted(n for n in inert if n in best) or 'none'}" + (f"; below 10 RTOL in Float32: {sorted(weak_f32)}" if weak_f32 else ""))
        assert not weak, f"{fam} {ft}: parameters the states do not see (liveness < {S.MIN_LIVE}) and INERT does not name: {weak}"
        assert not stale, f"{fam} {ft}: INERT names parameters that are live: {stale}"
        assert all(n in best for n in inert), f"{fam} {ft}: INERT names parameters no entry reads: {[n for n in inert if n not in best]}"


# ---- the Chen-2022 fit boundary (host twin of tests/test_param_sweep_gpu.py::test_chen2022_fit_boundary) ------------------------------------------------
@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("which", ["2-moment", "sedimentation"])
def test_chen2022_fit_boundary(host, oracle, ft, which):
    """Whichever instantiation the host-side fit picks along the two walks (param_sweep.chen_boundary_cases) meets the bound; the harness's return code says
    which one ran (2-moment: bit 1; sedimentation: 1), printed per step — Float64's acceptance (2e-14 on the fitted logarithm) gives way to the general kernel
    earlier than Float32's."""
    e = S.SbTendencies(True, "chen") if which == "2-moment" else S.Sedimentation()
    picked = {}

    probe, out = S.chen_density_probe(e, ft)

    def runner(p, x, label):
        rc, y = e.host(host, p, x, ft)
        assert rc >= 0, (label, rc)
        picked[label] = S.chen_host_is_general(e, rc)
        v = e.host(host, p, probe, ft)[1][out]                  # ρ = 2.5: NaN from the fitted instantiation only
        assert np.all(np.isfinite(v)) if picked[label] else np.all(np.isnan(v)), (label, v[:4])
        return y
    sweep = S.run_cases(e, ft, runner, S.chen_boundary_cases())
    for label, general in picked.items():
        print(f"[Chen-2022 boundary, host] {which} {ft}: {label}: {'general (run-time Γ)' if general else 'fitted'}")
    assert not picked["defaults"]
    assert picked[[k for k in picked if k.startswith("b_rho")][-1]] and picked[[k for k in picked if k.startswith("b[2]")][-1]]
    sweep.finish()


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_sb2006_fall_speed_needs_aR_below_bR(host, oracle, ft):
    """Host twin of the device test: aR = 0.999 bR meets the bound with the not-limited PSD on states with q_rai = 0 at N_rai > ϵ (and the converse); aR ≥ bR is
    refused there (CMX_ERR_BAD_ARG) and accepted by the limited PSD and by the Chen-2022 speed.  The oracle shows why: with aR > bR it returns the reference's NaN (Float64 gates) at such states with many drops."""
    x = S.aR_states(ft)
    nl, lim, chen = S.SbTendencies(False, "sb"), S.SbTendencies(True, "sb"), S.SbTendencies(False, "chen")

    def run(e):
        def runner(p, x_, label):
            rc, y = e.host(host, p, x_, ft)
            assert rc >= 0, (label, rc)
            return y
        return runner
    sweep = S.run_cases(nl, ft, run(nl), [("aR = 0.999 bR", S.aR_override(0.999))], x=x)
    for f in (1.0, 1.03):
        ov = S.aR_override(f)
        assert nl.host(host, nl.params(P.ParamDict(ft, ov)), x[0], ft)[0] == _abi.CMX_ERR_BAD_ARG
        if f > 1 and ft == "f64":       # r_c < 0: exp(−2 r_c λ_r) overflows once λ_r = (π ρ_w N/(ρ ϵ))^⅓ is large enough — with ϵ = eps(Float64), from N_rai ≈ 1e5 per kg
            ref = nl.ref(nl.params(P.ParamDict("f64", ov)), x[1], ft)
            at_risk = (x[1][5] == 0) & (x[1][6] > 1e6)
            assert at_risk.sum() > 20 and np.all(np.isnan(ref["vt_rai_n"][at_risk])), "the reference's Inf − Inf, restated by the oracle"
        for e in (lim, chen):
            S.run_cases(e, ft, run(e), [(f"aR = {f:g} bR, {e}", ov)], sweep=sweep, x=x)
    sweep.finish()


def test_weak_f32_rows_cannot_reach_the_threshold(oracle):
    """A WEAK_F32 row is a claim that NO state of the family makes the parameter visible at 10·RTOL[f32] = 1 % — directed states could not help.  Checked on the
    oracle over states far wider than the sweep's (L = 1e-7…3e-2 kg/m³, N = 0.1…1e7 1/m³: the shape solve runs into its lower bracket log λ = 2)."""
    rng = np.random.default_rng(5)
    m = 600
    x = [10 ** rng.uniform(-7, -1.5, m), 10 ** rng.uniform(-1, 7, m), rng.uniform(0, 0.95, m), rng.uniform(200, 800, m), rng.uniform(0.4, 1.3, m),
         rng.uniform(274, 300, m)]
    for name in S.WEAK_F32["P3"]:
        worst = 0.0
        for e in (S.P3Velocities(), S.P3SelfCollection(), S.P3Melt()):
            r0 = e.ref(e.params(P.ParamDict("f64")), x, "f32")
            for c in S.perturbations([name])[0]:
                r = e.ref(e.params(P.ParamDict("f64", c.override)), x, "f32")
                for k in e.names:
                    with np.errstate(all="ignore"):
                        rel = np.abs(r[k] - r0[k]) / np.abs(r0[k])
                    worst = max(worst, float(np.max(np.where(np.isfinite(rel), rel, 0.0))))
        print(f"[weak in Float32] P3 {name}: largest relative movement of any P3 integral {worst:.4f}")
        assert worst < S.LIVE_FACTOR * parity.RTOL["f32"], (name, worst)


def test_float32_domain_rows_of_the_nucleation_rates():
    """The two Float32 DOMAIN rows: the reference's own Float32 arithmetic (term by term, as Nucleation.jl:51-90 writes it) is non-finite at every state there; and
    at the defaults and at every other perturbation of the entry it leaves the range at no more states than the cap on exclusions allows."""
    e = S.AerosolNucleation()
    x64 = e.states("f32")[1]
    cases, skipped = S.perturbations(e.read(), ("Float32",))
    assert sorted(c.key for c in skipped) == ["mam3_nucleation_v_t_n_neutral x0.8", "mam3_nucleation_w_t_n_neutral x0.8"]
    for c in skipped:
        p = e.params(P.ParamDict("f64", c.override))
        h, a, ion, T = x64[0], x64[1], x64[2], x64[6]
        assert not np.isfinite(e._ternary_literal_f32(e.params(P.ParamDict("f32", c.override))["hp"], h, a, ion, T)).any(), c.key
    worst = max(int(e.ref(e.params(P.ParamDict("f64", c.override)), x64, "f32")["near_branch"].sum()) for c in cases)
    print(f"[Float32 range] nucleation_rates: at most {worst} of {x64[0].size} states set aside per perturbation")
    assert worst <= 2
