"""CPU tests: the oracle's P3 shape solve against high-precision roots of the shape equation (tests/golden/p3_shape_roots.json,
written by tools/gen_p3_shape_roots.py from tests/p3_shape_hp.py — mpmath, exact incomplete gamma functions, every root on [2, 17]).

The oracle (oracle/cmx_oracle_p3_impl.h) is the reference's stand-in for the device tests, and until now it was only compared with
restatements by the same hand.  Here it is tested first against an equation that shares none of its code: a wrong segment bound,
mass-law coefficient, P/Q choice, eps floor or μ(λ) moves its root away from the true one.  Tolerances are parity.RTOL.  The
device runs the same fixture in tests/test_p3_shape_roots_gpu.py."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
if str(REPO / "tools") not in sys.path:
    sys.path.insert(0, str(REPO / "tools"))

import gen_p3_shape_roots as gen  # noqa: E402
import parity  # noqa: E402
from cmx import _abi  # noqa: E402
from cmx import parameters as P  # noqa: E402

RTOL = parity.RTOL
MIN_CONVERGED_SHARE = 0.88


@pytest.fixture(scope="module")
def fx():
    return gen.load()


def test_fixture_is_what_its_generator_writes():
    r = subprocess.run([sys.executable, str(REPO / "tools" / "gen_p3_shape_roots.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_fixture_covers_its_strata(fx):
    S = fx["states"]
    n = {k: sum(s["s"] == k for s in S) for k in gen.NOTES}
    assert n["random"] >= 300 and n["band"] >= 60 and n["fold"] >= 50 and n["fold-edge"] >= 20 and n["constant-slope"] >= 30, n
    assert (REPO / "tests" / "golden" / "p3_shape_roots.json").stat().st_size < 400_000
    for s in S:
        for e in ("f64", "f32"):
            r = s[e]
            if s["s"] == "fold":
                assert len(r["roots"]) == 3, s
            if s["s"] == "constant-slope":
                assert len(r["roots"]) == 1 and r["roots"][0][3] < 0, s        # monotonic: one root, f decreasing
            if s["s"] == "band":
                assert any(8 <= row[0] < 11 for row in r["roots"]), s
    ends = [s["f64"]["end"] for s in S if "end" in s["f64"]]
    assert 2 in ends and 17 in ends
    assert any("absent" in s["f32"] and "roots" in s["f64"] for s in S)          # between the two gates
    assert any(len(s["f64"]["roots"]) == 2 or len(s["f64"]["roots"]) == 3 for s in S if s["s"] == "fold-edge")
    h = fx["header"]["oracle_alone"]
    assert h["worst_forward_error_80_evaluations_f64_gates"] <= RTOL["f64"] and h["worst_forward_error_80_evaluations_f32_gates"] <= RTOL["f64"]
    assert h["converged_share_random_f64"] >= MIN_CONVERGED_SHARE and h["converged_share_random_f32"] >= MIN_CONVERGED_SHARE


def check_against_roots(S, e, out, rtol, what):
    """Every state of S against its entry for eps type e: −Inf without ice, the recorded end exactly where there is no sign change,
    else within rtol of SOME true root, with D_m and log N₀ inside the bounds propagated from that root.  Returns the worst errors."""
    ll, Dm, lN0 = out["log_lambda"], out["D_m"], out["log_N0"]
    worst = {"log_lambda": 0.0, "D_m": 0.0, "log_N0": 0.0}
    for i, s in enumerate(S):
        r = s[e]
        if "absent" in r:
            assert ll[i] == -math.inf, (what, i, s, ll[i])
        elif "end" in r:
            assert ll[i] == float(r["end"]), (what, i, s, ll[i])
        else:
            err, row = gen.nearest_root(ll[i], r)
            assert err <= rtol, (what, i, s["s"], ll[i], r["roots"], err)
            b_dm, b_n0 = gen.propagated_bounds(row, rtol)
            e_dm, e_n0 = abs(Dm[i] / row[1] - 1), abs(lN0[i] - row[2])
            assert e_dm <= b_dm and e_n0 <= b_n0, (what, i, s["s"], e_dm, b_dm, e_n0, b_n0)
            worst = {"log_lambda": max(worst["log_lambda"], err), "D_m": max(worst["D_m"], e_dm / (b_dm / rtol)), "log_N0": max(worst["log_N0"], e_n0 / (b_n0 / rtol))}
    return worst


@pytest.mark.parametrize("gates", ["f64", "f32"])
def test_oracle_at_80_evaluations_finds_a_true_root(oracle, fx, gates):
    """Float64 arithmetic, converged: within RTOL[f64] of a true root for both gate types (the Float32-gated run against the roots of
    the 2⁻²³ floor).  Measured 1.2e-13 over the full fixture (header: worst_forward_error_80_evaluations_*)."""
    S = fx["states"]
    out = gen.oracle_loglambda(oracle, S, gates, maxiters=80, want=("log_lambda", "D_m", "log_N0"))
    worst = check_against_roots(S, gates, out, RTOL["f64"], f"oracle Float64, {gates} gates, 80 evaluations")
    print(f"\n[P3 roots] oracle Float64 arithmetic, {gates} gates, 80 evaluations: worst (normalised to its bound) {worst}")
    assert worst["log_lambda"] <= 10 * fx["header"]["oracle_alone"][f"worst_forward_error_80_evaluations_{gates}_gates"]   # a regression pin beside the RTOL above


def test_oracle_in_float32_arithmetic_finds_a_true_root(oracle, fx):
    S = fx["states"]
    out = gen.oracle_loglambda(oracle, S, "f32", arith="f32", maxiters=40, want=("log_lambda", "D_m", "log_N0"))
    worst = check_against_roots(S, "f32", out, RTOL["f32"], "oracle Float32 arithmetic, 40 evaluations")
    print(f"\n[P3 roots] oracle Float32 arithmetic, 40 evaluations: worst (normalised to its bound) {worst}")


@pytest.mark.parametrize("arith", ["f64", "f32"])
def test_fixed_term_counts_of_gamma_inc(oracle, fx, arith):
    """UT.gamma_inc runs a fixed 30 (Float64) / 20 (Float32) terms of its series or continued fraction.  How far that is from the exact
    function over the (z, x) the fixture visits — z = b + n + μ + 1, b ∈ {3, β_va}, n ∈ {0, 1}, μ ∈ [0, 6]; x = D·λ at the segment
    bounds, and x = z + 1 ∓ 1e-3 where the two expansions meet — is recorded in the fixture's header (1.3e-11 at 30 terms, 2.4e-6 at
    20 terms in Float32 arithmetic, absolute).  Asserted: the resulting residual at the true roots is within RTOL, nothing tighter."""
    S = [s for s in fx["states"] if "roots" in s[arith]]
    a, r = gen.gamma_inc_distance(oracle, gen.visited_gamma_arguments(S[::6], arith), arith)
    rec = fx["header"]["oracle_alone"][f"gamma_inc_{30 if arith == 'f64' else 20}_terms_{arith}_arithmetic"]
    print(f"\n[P3 roots] gamma_inc {arith}: worst |ΔP| {a:.2e} (header {rec['worst_abs_P_or_Q']:.2e}), worst relative error of the smaller of P, Q {r:.2e}")
    assert a <= RTOL[arith] and a <= 1.5 * rec["worst_abs_P_or_Q"]
    fam = {"f64": _abi.F64, "f32": _abi.F32}[arith]
    worst = 0.0
    for s in S:
        p = P.ParametersP3(arith, s["slope"])
        t = math.log(s["L"]) - math.log(s["N"])
        for row in s[arith]["roots"]:
            res = oracle.p3_logLdivN(fam, p.c, p.flags, s["F"], s["rr"], row[0]) - t
            worst = max(worst, abs(res))
    print(f"[P3 roots] oracle residual ({arith} arithmetic, fixed term count) at the true roots: worst {worst:.2e}")
    assert worst <= RTOL[arith]


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_converged_sets_at_the_reference_budget(oracle, fx, ft):
    """The converged set of a float type: the oracle alone (Float64 arithmetic, ft's gates, 10 / 8 evaluations) within RTOL/2 of a true
    root.  The fixture's flags are these, and the set holds at least 0.88 of the random stratum (0.929 / 0.913 on 100 000 states)."""
    S = fx["states"]
    ll = gen.oracle_loglambda(oracle, S, ft, maxiters=gen.BUDGET[ft])["log_lambda"]
    err = gen.forward_errors(ll, S, ft)
    k = {"f64": 0, "f32": 1}[ft]
    for i, s in enumerate(S):
        if s["conv"][k]:
            assert err[i] <= RTOL[ft] / 2 * 1.001, (i, s["s"], err[i])
        else:
            assert not err[i] <= RTOL[ft] / 2 * 0.999, (i, s["s"], err[i])
    rnd = [i for i, s in enumerate(S) if s["s"] == "random" and "roots" in s[ft]]
    share = np.mean([S[i]["conv"][k] for i in rnd])
    print(f"\n[P3 roots] converged set {ft}: {share:.4f} of {len(rnd)} random states; {sum(s['conv'][k] for s in S)} of {len(S)} states in all")
    assert share >= MIN_CONVERGED_SHARE


def test_brent_variants_are_told_apart(oracle, fx):
    """The evidence for the Zeroin restatement that csrc/cmx_p3.hpp cites: the Wikipedia-pseudo-code variant (1) fails the reference's
    warm-start suite that Brent's zeroin (0) passes, and at the reference budget the two land on different log λ in the band stratum."""
    from test_reference_suites import FAM, STATE, check_warmstart
    band = [s for s in fx["states"] if s["s"] == "band"]

    def solve_with(ft):
        p = P.ParametersP3(ft)
        return lambda cols, guess: oracle.p3_shape(FAM[ft], p.c, STATE | p.flags, *cols, guess=guess)["log_lambda"]
    try:
        oracle.set_brent_variant(1)
        for ft in ("f64", "f32"):
            with pytest.raises(AssertionError):
                check_warmstart(solve_with(ft), ft)
        ll1 = gen.oracle_loglambda(oracle, band, "f64", maxiters=gen.BUDGET["f64"])["log_lambda"]
    finally:
        oracle.set_brent_variant(0)
    for ft in ("f64", "f32"):
        check_warmstart(solve_with(ft), ft)
    ll0 = gen.oracle_loglambda(oracle, band, "f64", maxiters=gen.BUDGET["f64"])["log_lambda"]
    differ = np.abs(ll1 - ll0) > RTOL["f64"] * np.abs(ll0)
    print(f"\n[P3 roots] Brent variants 0 / 1 at 10 evaluations differ beyond RTOL on {int(differ.sum())} of {len(band)} band states (worst {np.abs(ll1 - ll0).max():.2e})")
    assert differ.any()
