"""The parameter sweep on the device (-m gpu; machinery, entries, states and the domain / inert tables: tests/param_sweep.py).

Every other GPU parity test runs the kernels at the ClimaParams defaults.  Here each parameter that a family's constructors read is changed alone (× 1.25, × 0.8;
a default of 0 by an additive step; tables element by element) and the caller-visible Python wrapper is compared with the oracle evaluated with the same
override in Float64 and the float type's gates, on the inputs as the float type rounds them — at parity.RTOL / CTOL with the DEFAULT knobs.  A folded constant
that ignores its field, or a fast instantiation selected by too few fields, fails here by name; tests/test_param_sweep_host.py proves on the oracle alone that
every case can see its parameter (≥ 50 states move by more than 10·RTOL).  One test per entry and float type; every failing (entry, parameter, direction) is
listed at once, and one summary row per entry and float type goes to the parity report.

Families: SB2006 (fused tendencies limited / not limited × SB / Chen velocity, process rates, cloud fall speed, the column step with cloud sedimentation, the
four bulk cloud-to-rain schemes, the susceptibilities), 1-moment (Instantaneous with the four option sets, LinearizedAverage, the source terms, the fall-speed
entries incl. snow_terminal_velocity with the fixed aspect ratio, Oblate and Prolate, the column step), 0-moment, cloud diagnostics, ice nucleation (ABIFM / Koop,
water activities, H2SO4 solution, deposition_J, Mohler), ARG2000 (mode descriptors and columns), aerosol nucleation (the fused rates against
tests/nucleation_ref.py with the perturbed structs), P3 on 515 states: p3_shape(brent_iters = 40) itself — log λ and D_m against the oracle's converged solve
with the same perturbed struct, a disagreeing state set aside only where the ORACLE's residual at the device's log λ vanishes (another root of the multi-root
band), within the cap on exclusions — and p3_terminal_velocities, p3_ice_self_collection, p3_ice_melt, each evaluated by the oracle at the log λ the device
solved for (those three therefore test the integrals, not the solve: that is p3_shape's entry).

Left out: the P3 collision sweeps and the fused 2M + P3 entry (seconds per perturbation); the parcel tendencies (tests/parcel_ref.py builds its parameter set
from the default structs); ARG2000's ice-sink method (its own test conditions S_max's numerator); INP_concentration_frequency (its own test allows 10·RTOL:
exp(−Δ²/2σ²) ten deviations out — so Frostenberg's σ is swept nowhere)."""
import numpy as np
import pytest
import torch

import param_sweep as S
import parity
from cmx import parameters as P

pytestmark = pytest.mark.gpu
ENTRIES = S.all_entries()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch.device("cuda:0")


def _to(x, dev):
    return [torch.from_numpy(c).to(dev) for c in x]


@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("k", range(len(ENTRIES)), ids=[str(e).replace(" ", "_") for e in ENTRIES])
def test_entry(dev, oracle, ft, k):
    e = ENTRIES[k]
    xt = _to(e.states(ft)[0], dev)
    sweep, live, skipped = S.run_sweep(e, ft, lambda p, x: e.gpu(p, xt))
    dead = sum(1 for v in live.values() if v == 0)
    print(f"[parameter sweep] {e} {ft}: {len(live)} perturbations ({dead} the oracle does not see here{', not launched' if e.skip_dead else ''}), "
          f"{len(skipped)} outside the domain")
    sweep.finish()


# ---- the Chen-2022 fit boundary ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    """the host build of the point functions: its return code names the instantiation that chen_vel_kind / make_chen_gamma pick (the device entry reports CMX_OK only)"""
    import ctypes as C
    import subprocess
    from pathlib import Path
    repo = Path(__file__).resolve().parent.parent
    out = repo / "tests" / "native" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libparam_sweep_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(repo / "tests" / "native" / "point_host.cpp")], check=True)
    return C.CDLL(str(so))


@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("which", ["2-moment", "sedimentation"])
def test_chen2022_fit_boundary(dev, host, oracle, ft, which):
    """b_ρ from Table B1's 0.038 to 0.6, and b₃ down to the pole guard b₃ + 1 − 2 b_ρ = 0.05, in 12 geometric steps each: whichever instantiation chen_vel_kind /
    make_chen_gamma picks meets the same bound against the oracle.  Which one that is comes from the host-side selection (the harness's return code, the same
    functions the entries call), printed per step; and at EVERY step ρ = 2.5 gives NaN fall speeds on the device if and only if that selection is the fitted one —
    'ρ > 2 gives NaN from the fitted kernels only', tested against an independent label."""
    e = S.SbTendencies(True, "chen") if which == "2-moment" else S.Sedimentation()
    xt = _to(e.states(ft)[0], dev)
    probe, out = S.chen_density_probe(e, ft)
    probe_t = _to(probe, dev)
    picked = {}

    def runner(p, x, label):
        rc, _ = e.host(host, p, [c[:8] for c in x], ft)
        assert rc >= 0, (label, rc)
        picked[label] = S.chen_host_is_general(e, rc)
        v = e.gpu(p, probe_t)[out]
        assert np.all(np.isfinite(v)) if picked[label] else np.all(np.isnan(v)), (label, "general" if picked[label] else "fitted", v[:4])
        return e.gpu(p, xt)
    sweep = S.run_cases(e, ft, runner, S.chen_boundary_cases())
    for label, general in picked.items():
        print(f"[Chen-2022 boundary] {which} {ft}: {label}: {'general (run-time Γ)' if general else 'fitted'}")
    assert not picked["defaults"], "Table B1 itself takes the fitted instantiation"
    assert picked[[k for k in picked if k.startswith("b_rho")][-1]] and picked[[k for k in picked if k.startswith("b[2]")][-1]], "the ends of both walks are general"
    sweep.finish()


# ---- aR ≥ bR ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_sb2006_fall_speed_needs_aR_below_bR(dev, oracle, ft):
    """The SB2006 fall speed of the NOT-limited PSD integrates from r_c = −log(aR/bR)/(2cR).  With aR ≥ bR the reference returns NaN wherever q_rai = 0 at
    N_rai > ϵ (exp(−2 r_c λ_r) overflows; src/Microphysics2M.jl:685-739) — the entries that evaluate it refuse such a struct (CMX_ERR_BAD_ARG, include/cmx.h
    Conventions) instead of returning a number.  aR just below bR is in the domain and meets the bound on exactly those states; the limited PSD and the Chen-2022
    speed take any aR, bR."""
    import cmx
    x = S.aR_states(ft)
    xt = _to(x[0], dev)
    nl, lim, chen = S.SbTendencies(False, "sb"), S.SbTendencies(True, "sb"), S.SbTendencies(False, "chen")
    sweep = S.run_cases(nl, ft, lambda p, x_, label: nl.gpu(p, xt), [("aR = 0.999 bR", S.aR_override(0.999))], x=x)
    for f in (1.0, 1.03):
        ov = S.aR_override(f)
        with pytest.raises(cmx.CmxStatusError):
            nl.gpu(nl.params(P.ParamDict(ft, ov)), xt)
        pr = S.SbProcessRates(False)
        with pytest.raises(cmx.CmxStatusError):
            pr.gpu(pr.params(P.ParamDict(ft, ov)), _to(pr.states(ft)[0], dev))
        col = S.SbColumn(False, "sb")
        with pytest.raises(cmx.CmxStatusError):
            col.gpu(col.params(P.ParamDict(ft, ov)), _to(col.states(ft)[0], dev))
        for e in (lim, chen):
            S.run_cases(e, ft, lambda p, x_, label, e=e: e.gpu(p, xt), [(f"aR = {f:g} bR, {e}", ov)], sweep=sweep, x=x)
    sweep.finish()
