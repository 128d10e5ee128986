"""GPU tests: the p3_shape kernel against high-precision roots of the shape equation (tests/golden/p3_shape_roots.json; the equation is
tests/p3_shape_hp.py, the oracle is tested against the same file in tests/test_p3_shape_roots.py).  No oracle is needed here: an error
that csrc/cmx_p3.hpp shares with oracle/cmx_oracle_p3_impl.h cannot hide.

Criteria, per state and float type ft, against the roots of ft's eps floor:
  forward    |log λ − r| ≤ RTOL[ft]·|r| for SOME true root r;
  backward   |f(log λ)| ≤ RTOL[ft] with f the high-precision residual: the device's λ is exact for an L/N perturbed by no more than the
             north-star tolerance.  It is the looser of the two only where |f′(r)|·|r| < 1, so it is open to the fold and fold-edge
             strata and to the states with such a root (the fixture's ∂f/∂logλ), and to nobody else.
No state is set aside."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
if str(REPO / "tools") not in sys.path:
    sys.path.insert(0, str(REPO / "tools"))

import gen_p3_shape_roots as gen  # noqa: E402
import p3_shape_hp as hp  # noqa: E402
import parity  # noqa: E402
from cmx import parameters as P  # noqa: E402

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
RTOL = parity.RTOL
ALL = ("F_rim", "rho_rim", "log_lambda", "D_m", "log_N0")
FAMILY = "P3 shape solve (a5)"
PINNED_BY = "high-precision roots of the shape equation (tests/golden/p3_shape_roots.json)"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return gen.load()


def solve(dev, S, ft, brent_iters=0, guess=None):
    """cmx.p3_shape(…, from_state=True, want=ALL) over the fixture: one launch for the power-law states, one for the constant-slope ones."""
    import cmx
    out = {k: np.full(len(S), np.nan) for k in ("log_lambda", "D_m", "log_N0")}
    for slope in ("powerlaw", "constant"):
        idx = [i for i, s in enumerate(S) if s["slope"] == slope]
        cols = [torch.tensor(c, dtype=DT[ft], device=dev) for c in gen.columns([S[i] for i in idx])]
        g = None if guess is None else torch.tensor(np.asarray(guess)[idx], dtype=DT[ft], device=dev)
        r = cmx.p3_shape(P.ParametersP3(ft, slope), *cols, from_state=True, want=ALL, brent_iters=brent_iters, log_lambda_guess=g)
        assert torch.equal(r.F_rim, cols[2]) and torch.equal(r.rho_rim, cols[3])
        for k in out:
            out[k][idx] = getattr(r, k).cpu().numpy().astype(np.float64)
    return out


_STATES = {}


def hp_residual(s, ft, x):
    key = (s["slope"], s["F"], s["rr"])
    if key not in _STATES:
        _STATES[key] = hp.state(gen._params(s["slope"]), s["F"], s["rr"], s["slope"])
    return float(hp.residual(_STATES[key], s["L"], s["N"], x, hp.EPS[ft]))


def backward_allowed(s, ft):
    return s["s"] in ("fold", "fold-edge") or any(abs(row[3]) * abs(row[0]) < 1 for row in s[ft]["roots"])


def judge(S, ft, out, what, only=None):
    """The criteria above for every state (or those of `only`).  Returns (mask of forward passes, nearest rows, forward errors, report)."""
    ll = out["log_lambda"]
    n = len(S)
    fwd, rows, err = np.zeros(n, dtype=bool), [None] * n, np.full(n, np.nan)
    rep = {}
    for i, s in enumerate(S):
        if only is not None and not only[i]:
            continue
        r = s[ft]
        if "absent" in r:
            assert ll[i] == -math.inf, (what, i, s, ll[i])
            continue
        if "end" in r:
            assert ll[i] == float(r["end"]), (what, i, s, ll[i])
            continue
        assert math.isfinite(ll[i]) and 2 <= ll[i] <= 17, (what, i, s, ll[i])
        err[i], rows[i] = gen.nearest_root(ll[i], r)
        st = rep.setdefault(s["s"], {"n": 0, "forward": 0, "backward": 0, "worst_forward": 0.0, "worst_backward": 0.0})
        st["n"] += 1
        if err[i] <= RTOL[ft]:
            fwd[i] = True
            st["forward"] += 1
            st["worst_forward"] = max(st["worst_forward"], float(err[i]))
            continue
        assert backward_allowed(s, ft), (what, "a well-conditioned state misses every true root", i, s["s"], ll[i], r["roots"], err[i])
        res = abs(hp_residual(s, ft, ll[i]))
        st["backward"] += 1
        st["worst_backward"] = max(st["worst_backward"], res)
        assert res <= RTOL[ft], (what, "neither a root nor a small residual", i, s["s"], ll[i], r["roots"], err[i], res)
    return fwd, rows, err, rep


def check_moments(S, ft, out, fwd, rows, what):
    """D_m and log N₀ of the forward-passing states inside the bounds propagated from their root (no 20 × RTOL)."""
    worst = {"D_m": 0.0, "log_N0": 0.0}
    for i in np.flatnonzero(fwd):
        b_dm, b_n0 = gen.propagated_bounds(rows[i], RTOL[ft])
        e_dm, e_n0 = abs(out["D_m"][i] / rows[i][1] - 1), abs(out["log_N0"][i] - rows[i][2])
        worst = {"D_m": max(worst["D_m"], e_dm / b_dm), "log_N0": max(worst["log_N0"], e_n0 / b_n0)}
        assert e_dm <= b_dm and e_n0 <= b_n0, (what, i, S[i]["s"], S[i], out["log_lambda"][i], rows[i], e_dm, b_dm, e_n0, b_n0)
    return worst


def record(S, ft, out, fwd, rows, what, note):
    ref = {k: np.array([rows[i][j] if fwd[i] else np.nan for i in range(len(S))]) for j, k in enumerate(("log_lambda", "D_m", "log_N0"))}
    parity.record(what, ft, out, ref, family=FAMILY, pinned_by=PINNED_BY, keep=fwd, scale={"log_N0": np.ones(len(S))}, note=note)


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_converged_budget_finds_a_true_root(dev, fx, ft):
    S = fx["states"]
    out = solve(dev, S, ft, brent_iters=40)
    what = f"P3 roots {ft} brent_iters=40"
    fwd, rows, err, rep = judge(S, ft, out, what)
    worst = check_moments(S, ft, out, fwd, rows, what)
    print(f"\n[{what}] per stratum {rep}\n[{what}] D_m / log N0, worst share of the propagated bound: {worst}")
    record(S, ft, out, fwd, rows, what, f"{int(fwd.sum())} states within RTOL of a true root; the others pass the backward criterion: {({k: v['backward'] for k, v in rep.items() if v['backward']})}")


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_reference_budget_on_the_converged_set(dev, fx, ft):
    """Where the oracle alone reaches RTOL/2 of a true root at the reference's 10 / 8 evaluations (the fixture's flags), the device is within
    the plain RTOL of one.  The rest is reported: with the budget the reference fixes, nothing can be pinned there."""
    S = fx["states"]
    k = {"f64": 0, "f32": 1}[ft]
    out = solve(dev, S, ft)
    what = f"P3 roots {ft} reference budget"
    conv = np.array([bool(s["conv"][k]) for s in S])
    ll = out["log_lambda"]
    fwd, rows, err = np.zeros(len(S), dtype=bool), [None] * len(S), np.full(len(S), np.nan)
    for i, s in enumerate(S):
        r = s[ft]
        if "absent" in r:
            assert ll[i] == -math.inf, (what, i, s)
        elif "end" in r:
            assert ll[i] == float(r["end"]), (what, i, s, ll[i])
        else:
            assert math.isfinite(ll[i]) and 2 <= ll[i] <= 17, (what, i, s, ll[i])
            err[i], rows[i] = gen.nearest_root(ll[i], r)
            fwd[i] = err[i] <= RTOL[ft]
            if conv[i]:
                assert fwd[i], (what, "converged set", i, s["s"], ll[i], r["roots"], err[i])
    rest = ~conv & np.isfinite(err)
    in_band = rest & (ll >= 8) & (ll < 11)
    worst = check_moments(S, ft, out, fwd, rows, what)
    print(f"\n[{what}] converged set: {int(conv.sum())} states, worst forward error {np.nanmax(err[conv]):.2e}; the rest: {int(rest.sum())} states, "
          f"{int(in_band.sum())} of them in 8 <= log λ < 11, worst forward error {np.nanmax(err[rest]):.2e}; D_m / log N0 share of bound {worst}")
    record(S, ft, out, conv & fwd, rows, what, f"converged set of the oracle alone ({int(conv.sum())} states); {int(rest.sum())} further states are outside it and only reported")


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_warm_start_lands_on_a_true_root(dev, fx, ft):
    S = fx["states"]
    n = len(S)
    what = f"P3 roots {ft} warm start"
    cold = solve(dev, S, ft, brent_iters=40)
    for bad in (math.nan, 1.0, 18.0):                                 # not a usable guess: the cold bracket, bit for bit
        got = solve(dev, S, ft, brent_iters=40, guess=np.full(n, bad))
        for k in cold:
            assert np.array_equal(got[k], cold[k], equal_nan=True), (what, bad, k)
    base = np.array([s[ft]["roots"][0][0] if "roots" in s[ft] else 9.0 for s in S])
    rep = {}
    for d in (-1.0, -0.01, 0.01, 1.0):
        out = solve(dev, S, ft, brent_iters=40, guess=np.clip(base + d, 2.001, 16.999))
        fwd, rows, _, r = judge(S, ft, out, f"{what} guess = r{d:+g}")
        check_moments(S, ft, out, fwd, rows, f"{what} guess = r{d:+g}")
        rep[d] = {k: (v["forward"], v["backward"]) for k, v in r.items()}
    fold = np.array([s["s"] == "fold" for s in S])
    for j in range(3):                                                # each of the three roots of a fold state ± 0.01: a true root, whichever
        for d in (-0.01, 0.01):
            g = np.array([s[ft]["roots"][j][0] + d if s["s"] == "fold" else 9.0 for s in S])
            out = solve(dev, S, ft, brent_iters=40, guess=g)
            judge(S, ft, out, f"{what} fold root {j} {d:+g}", only=fold)
    print(f"\n[{what}] (forward, backward) passes per stratum and guess offset: {rep}")
