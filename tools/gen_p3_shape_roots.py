#!/usr/bin/env python3
"""Writes tests/golden/p3_shape_roots.json: high-precision roots of the P3 shape equation (tests/p3_shape_hp.py, mpmath) for about
600 states in strata chosen for where a shape solver goes wrong, and the oracle-alone statistics that the tests of
tests/test_p3_shape_roots.py re-derive.

  --write   solve every state (minutes; one process per core) and write the fixture
  --check   recompute a fixed subset of about 20 states, at least one per stratum, and compare with the committed file

Every input (L, N, F_rim, ρ_rim) is exactly representable in Float32, so the Float32 and the Float64 kernels solve the same
problem.  Per state and per eps (2⁻⁵² as "f64", 2⁻²³ as "f32"; "=" where the Float32-eps entry equals the Float64-eps one) the
file holds either {"roots": [[logλ, D_m, log N₀, ∂f/∂logλ, ∂ln D_m/∂logλ, ∂log N₀/∂logλ], …]} (every root on [2, 17],
ascending), {"end": 2 | 17, "sign": [sign f(2), sign f(17)]} (no sign change: the reference returns the end with the smaller
|f|) or {"absent": true} (L or N below the gate: log λ = −Inf).  "conv" = [Float64, Float32] membership of the converged set:
the ORACLE at the reference's Brent budget (Float64 arithmetic; 10 evaluations with Float64 gates, 8 with Float32 gates) lies
within RTOL/2 of a true root.  No device result enters the file.
"""
import argparse
import itertools
import json
import math
import multiprocessing
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
for _p in (REPO / "cloudmicrophysics.jl_amd", REPO / "oracle", REPO / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import mpmath as mp  # noqa: E402

import p3_shape_hp as hp  # noqa: E402

OUT = REPO / "tests" / "golden" / "p3_shape_roots.json"
RTOL = {"f64": 1e-6, "f32": 1e-3}                       # tests/parity.py
BUDGET = {"f64": 10, "f32": 8}                          # src/P3_size_distribution.jl:311
N_RANDOM, SEED_RANDOM, N_CONSTANT, SEED_CONSTANT = 320, 99, 30, 5
NOTES = {
    "random": "synthetic.p3_state(seed 99) in state form (F_rim = q_rim/L, ρ_rim = q_rim/b_rim), rounded to Float32; 1 % have no ice",
    "band": "a root in 8 ≤ log λ < 11, where μ(λ) ramps from 0 to 6 and the fixed Brent budget is short",
    "fold": "three roots: log(L/N) inside the rising window of logLdivN (between its local minimum at the μ = 0 kink and its local "
            "maximum).  |f′|·|r| < 1 at the roots on the rising branch: backward criterion allowed",
    "fold-edge": "log(L/N) within 1e-4 / 1e-6 of the local maximum or minimum of logLdivN, on either side: nearly double roots, or a "
                 "near-touch beside a single root.  |f′| → 0 at the maximum: backward criterion allowed",
    "rime-edge": "F_rim ∈ {0, 1e-8, 1e-3, 0.95, 0.99, 1 − 2⁻²³} × ρ_rim ∈ {50, 200, 800, 900}; D_gr within 1e-3 of D_th with D_cr "
                 "enormous (ρ_rim = 916, F_rim = 1 − 2⁻²³) and D_gr below D_th (ρ_rim = 950, F_rim = 0.99); the regression state and "
                 "every 7th state of the robustness sweep of tests/golden/p3_kats.json",
    "bracket-end": "no sign change on [2, 17], on both sides, with N or L (or both) just above the absent-ice gate; and two states "
                   "whose L lies between the Float64 and the Float32 gate (ice for one float type, none for the other)",
    "constant-slope": "SlopeConstant (μ = 0): the residual is monotonic, one root each",
}


def f32(x):
    return float(np.float32(x))


def _params(slope="powerlaw"):
    from cmx import parameters as P
    return hp.params_from(P.ParametersP3("f64", slope).c)


def _synthetic(n, seed):
    import torch
    from cmx import synthetic
    st = synthetic.p3_state(n, dtype=torch.float64, seed=seed)          # as tests/test_p3_gpu.py::_columns(…, from_state=True)
    F = torch.where(st.rho_q_ice > 0, st.rho_q_rim / st.rho_q_ice.clamp(min=1e-300), torch.zeros_like(st.rho_q_ice))
    rr = torch.where(st.rho_b_rim > 0, st.rho_q_rim / st.rho_b_rim.clamp(min=1e-300), torch.full_like(F, 400.0))
    return [c.to(torch.float32).to(torch.float64).numpy() for c in (st.rho_q_ice, st.rho_n_ice, F, rr)]


def _pair_for(t, rng_key):
    """A Float32 pair (L, N) whose log(L/N) is as close to t as Float32 allows, from 400 candidate N."""
    best = None
    for k in range(400):
        N = f32(10.0 ** (3 + (rng_key % 3)) * (1 + k / 997.0))
        L = f32(N * math.exp(t))
        d = abs(math.log(L) - math.log(N) - t)
        if best is None or d < best[0]:
            best = (d, L, N)
    return best[1], best[2]


def _fold_targets(args):
    F, rr = args
    st = hp.state(_params(), F, rr)
    return (F, rr), [(float(x), float(g), k) for x, g, k in hp.extrema(st, hp.EPS["f64"])]


def build_states():
    """The inputs, deterministically (the fold strata take a high-precision scan of logLdivN per (F_rim, ρ_rim))."""
    S = []
    add = lambda s, L, N, F, rr, slope="powerlaw": S.append(   # noqa: E731
        {"s": s, "slope": slope, "L": f32(L), "N": f32(N), "F": f32(F), "rr": f32(rr)})
    for L, N, F, rr in zip(*_synthetic(N_RANDOM, SEED_RANDOM)):
        add("random", L, N, F, rr)
    rng = np.random.default_rng(2024)
    pr = _params()
    for i in range(60):                                              # band: the target is logLdivN at a drawn log λ in [8, 11)
        F = 0.0 if i % 3 == 0 else f32(rng.uniform(0.0, 0.95))
        rr = f32(rng.uniform(200.0, 800.0))
        x = rng.uniform(8.0, 11.0)
        t = float(hp.logLdivN(hp.state(pr, F, rr), x, hp.EPS["f64"]))
        N = f32(math.exp(rng.uniform(math.log(1e2), math.log(1e6))))
        add("band", N * math.exp(t), N, F, rr)
    combos = list(itertools.product((0.0, 0.3, 0.5, 0.9), (200.0, 400.0, 600.0)))
    with multiprocessing.Pool(min(8, multiprocessing.cpu_count())) as pool:
        ext = pool.map(_fold_targets, [(f32(F), rr) for F, rr in combos])
    for (F, rr), ex in ext:
        mins, maxs = [e for e in ex if e[2] == "min"], [e for e in ex if e[2] == "max"]
        if not (mins and maxs) or not mins[0][0] < maxs[0][0]:
            continue                                                 # no rising window for this rime state
        g_lo, g_hi = mins[0][1], maxs[0][1]
        for j in range(6):                                           # fold: strictly inside the window
            t = g_lo + (g_hi - g_lo) * (0.08 + 0.84 * rng.uniform())
            N = f32(math.exp(rng.uniform(math.log(1e2), math.log(1e6))))
            add("fold", N * math.exp(t), N, F, rr)
        if (F, rr) in ((0.0, 400.0), (f32(0.5), 400.0), (f32(0.3), 600.0)):
            for k, (g, d) in enumerate(itertools.product((g_hi, g_lo), (-1e-4, -1e-6, 1e-6, 1e-4))):
                add("fold-edge", *_pair_for(g + d, k), F, rr)
    LN = [(1e-4, 1e4), (2.366e-5, 16461.6), (1e-3, 1e3), (1e-6, 1e6), (3e-5, 2e5), (5e-4, 3e2)]
    for i, (F, rr) in enumerate(itertools.product((0.0, 1e-8, 1e-3, 0.95, 0.99, 1 - 2.0 ** -23), (50.0, 200.0, 800.0, 900.0))):
        add("rime-edge", *LN[i % len(LN)], F, rr)
    for L, N in LN[:3]:
        add("rime-edge", L, N, 1 - 2.0 ** -23, 916.0)                # D_gr ≈ D_th from above, D_cr enormous
        add("rime-edge", L, N, 0.99, 950.0)                          # ρ_g > ρ_i: D_gr < D_th, the dense-rimed segment is empty
    kats = json.loads((REPO / "tests" / "golden" / "p3_kats.json").read_text())
    e = kats["regression_state"]
    add("rime-edge", e["L_ice"], e["N_ice"], e["F_rim"], e["rho_rim"])
    sw = kats["robustness_sweep"]
    for L, N, F, rr in list(itertools.product(sw["L_ice"], sw["N_ice"], sw["F_rim"], sw["rho_rim"]))[::7]:
        add("rime-edge", L, N, F, rr)
    for F, rr in ((0.0, 400.0), (0.5, 400.0), (0.95, 800.0)):        # bracket ends; the gates are eps(FT) = 2⁻²³ / 2⁻⁵²
        add("bracket-end", 1e-3, 2e-7, F, rr)                        # N just above the gate, L/N enormous  → log λ = 2
        add("bracket-end", 2e-7, 2e-7, F, rr)                        # both just above the gate, L/N = 1    → log λ = 2
        add("bracket-end", 2e-7, 1e15, F, rr)                        # L just above the gate, L/N tiny      → log λ = 17
    add("bracket-end", 1e-8, 1e3, 0.0, 400.0)                        # 2⁻⁵² < L < 2⁻²³: ice for Float64, none for Float32
    add("bracket-end", 1e-9, 1e2, 0.5, 400.0)
    cols = _synthetic(400, SEED_CONSTANT)
    keep = [i for i in range(400) if cols[0][i] > 0][:N_CONSTANT]
    for i in keep:
        add("constant-slope", cols[0][i], cols[1][i], cols[2][i], cols[3][i], "constant")
    return S


def _fl(x):
    return float(x)


def _fl12(x):
    return float(f"{float(x):.12g}")              # the derivatives only scale tolerances


def solve_state(s):
    """The fixture entries {"f64": …, "f32": …} of one state."""
    st = hp.state(_params(s["slope"]), s["F"], s["rr"], s["slope"])
    sc = None
    out = {}
    for e in ("f64", "f32"):
        eps = hp.EPS[e]
        if not hp.has_ice(s["L"], s["N"], eps):
            out[e] = {"absent": True}
            continue
        sc = sc or hp.scan(st)
        r = hp.roots(st, s["L"], s["N"], eps, sc)
        if "end" in r:
            out[e] = {"end": r["end"], "sign": [r["sign_lo"], r["sign_hi"]]}
            continue
        rows = []
        for x in r["roots"]:
            df, ds, dt = hp.derivatives(st, s["L"], s["N"], x, eps)
            rows.append([_fl(x), _fl(hp.D_m(st, s["L"], s["N"], x, eps)), _fl(hp.log_N0(st, s["N"], x)), _fl12(df), _fl12(ds), _fl12(dt)])
        out[e] = {"roots": rows}
    if out["f32"] == out["f64"]:
        out["f32"] = "="
    return out


# ---- reading the fixture (shared with the tests) --------------------------------------------------------------------------------
def load(path=OUT):
    fx = json.loads(Path(path).read_text())
    for s in fx["states"]:
        s.setdefault("slope", "powerlaw")
        if s["f32"] == "=":
            s["f32"] = s["f64"]
    return fx


def columns(states):
    return [np.array([s[k] for s in states], dtype=np.float64) for k in ("L", "N", "F", "rr")]


def nearest_root(x, entry):
    """(relative distance to the nearest true root, its row) of a solver's log λ for one state entry with roots."""
    best = min(entry["roots"], key=lambda row: abs(x - row[0]))
    return abs(x - best[0]) / abs(best[0]), best


def propagated_bounds(row, rtol):
    """(bound on |D_m/D_m(r) − 1|, bound on |log N₀ − log N₀(r)|) for a log λ within rtol·|r| of the root r of `row`: the solver's own
    rtol plus the root's error carried through ∂ln D_m/∂logλ and ∂log N₀/∂logλ."""
    r, _, lN0, _, s, t = row
    return rtol * (1 + abs(s) * abs(r)), rtol * (max(abs(lN0), 1.0) + abs(t) * abs(r))


def oracle_loglambda(oracle, states, e, *, arith="f64", maxiters, guess=None, want=("log_lambda",)):
    """The oracle's outputs for `states` with the gates of float type e ("f64" | "f32"), in Float64 or Float32 arithmetic."""
    from cmx import _abi
    from cmx import parameters as P
    fam = {"f64": _abi.F64, "f32": _abi.F32}[arith]
    out = {k: np.full(len(states), np.nan) for k in want}
    for slope in ("powerlaw", "constant"):
        idx = [i for i, s in enumerate(states) if s["slope"] == slope]
        if not idx:
            continue
        p = P.ParametersP3(arith, slope)
        r = oracle.p3_shape(fam, p.c, _abi.CMX_P3_INPUT_IS_STATE | p.flags, *columns([states[i] for i in idx]),
                            guess=None if guess is None else np.asarray(guess)[idx], float32_gates=(e == "f32"), maxiters=maxiters)
        for k in want:
            out[k][idx] = r[k].astype(np.float64)
    return out


def forward_errors(ll, states, e):
    """Per state: relative distance of ll to the nearest true root (NaN for states without roots)."""
    err = np.full(len(states), np.nan)
    for i, s in enumerate(states):
        if "roots" in s[e]:
            err[i] = nearest_root(ll[i], s[e])[0]
    return err


def visited_gamma_arguments(states, e="f64"):
    """The (z, x) at which gamma_inc is evaluated at the true roots: z = b + n + μ + 1 for the law of each segment and n ∈ {0, 1},
    x = D·λ at the finite segment bounds — and, for every such z, x = z + 1 ∓ 1e-3 where the series hands over to the continued fraction."""
    pts = set()
    for s in states:
        if "roots" not in s[e]:
            continue
        st = hp.state(_params(s["slope"]), s["F"], s["rr"], s["slope"])
        for row in s[e]["roots"]:
            x = mp.mpf(row[0])
            mu, lam = hp.mu_of(st, x), mp.exp(x)
            for lo, hi, _, b in st.segments:
                for n in (0, 1):
                    z = float(b + n + mu + 1)
                    pts.update((z, float(D * lam)) for D in (lo, hi) if 0 < D < mp.inf)
                    pts.update(((z, z + 1 - 1e-3), (z, z + 1 + 1e-3)))
    return sorted(pts)


def gamma_inc_distance(oracle, pts, arith):
    """Worst |P_oracle − P| and worst relative error of the smaller of (P, Q) over pts, against mp.gammainc."""
    from cmx import _abi
    fam = {"f64": _abi.F64, "f32": _abi.F32}[arith]
    npt = {"f64": np.float64, "f32": np.float32}[arith]
    worst_abs = worst_rel = 0.0
    for z, x in pts:
        z, x = float(npt(z)), float(npt(x))
        P, Q = oracle.gamma_inc(fam, z, x)
        Pm = mp.gammainc(z, 0, x, regularized=True)
        Qm = mp.gammainc(z, x, mp.inf, regularized=True)
        worst_abs = max(worst_abs, abs(float(P - Pm)), abs(float(Q - Qm)))
        small, ref = (P, Pm) if Pm < Qm else (Q, Qm)
        if ref > 1e-30:
            worst_rel = max(worst_rel, abs(float((small - ref) / ref)))
    return worst_abs, worst_rel


def oracle_alone(oracle, states):
    """The header's statistics and the converged-set flags, from the oracle and the roots alone."""
    stats, flags = {}, {}
    for e in ("f64", "f32"):
        ll = oracle_loglambda(oracle, states, e, maxiters=80)["log_lambda"]
        stats[f"worst_forward_error_80_evaluations_{e}_gates"] = float(np.nanmax(forward_errors(ll, states, e)))
        ll = oracle_loglambda(oracle, states, e, maxiters=BUDGET[e])["log_lambda"]
        err = forward_errors(ll, states, e)
        flags[e] = [bool(v <= RTOL[e] / 2) for v in err]              # NaN (no roots) → False
        rnd = [i for i, s in enumerate(states) if s["s"] == "random" and "roots" in s[e]]
        stats[f"converged_share_random_{e}"] = float(np.mean([flags[e][i] for i in rnd]))
        stats[f"within_rtol_share_random_{e}"] = float(np.mean(err[rnd] <= RTOL[e]))
    ll = oracle_loglambda(oracle, states, "f32", arith="f32", maxiters=40)["log_lambda"]
    stats["worst_forward_error_float32_arithmetic_40_evaluations"] = float(np.nanmax(forward_errors(ll, states, "f32")))
    for arith, e in (("f64", "f64"), ("f32", "f32")):
        a, r = gamma_inc_distance(oracle, visited_gamma_arguments(states, e), arith)
        stats[f"gamma_inc_{30 if arith == 'f64' else 20}_terms_{arith}_arithmetic"] = {"worst_abs_P_or_Q": a, "worst_rel_smaller_of_P_Q": r}
    return stats, flags


def check_subset(states):
    """About 20 states: the first three of every stratum, spread over it."""
    pick = []
    for name in NOTES:
        idx = [i for i, s in enumerate(states) if s["s"] == name]
        pick += [idx[0], idx[len(idx) // 2], idx[-1]]
    return sorted(set(pick))


def _same(a, b, rtol=1e-12, dtol=1e-8):
    if a.keys() != b.keys():
        return False
    if "roots" not in a:
        return a == b
    if len(a["roots"]) != len(b["roots"]):
        return False
    for ra, rb in zip(a["roots"], b["roots"]):
        tol = (rtol, rtol, rtol, dtol, dtol, dtol)
        if any(abs(x - y) > t * max(abs(x), abs(y), 1e-300) for x, y, t in zip(ra, rb, tol)):
            return False
    return True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--write", action="store_true")
    g.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.check:
        fx = load()
        bad = []
        rnd = [s for s in fx["states"] if s["s"] == "random"]
        for s, (L, N, F, rr) in zip(rnd, zip(*_synthetic(N_RANDOM, SEED_RANDOM))):
            if (s["L"], s["N"], s["F"], s["rr"]) != (L, N, F, rr):
                bad.append(("random inputs", s))
        for s in fx["states"]:
            if any(f32(s[k]) != s[k] for k in ("L", "N", "F", "rr")):
                bad.append(("not a Float32 number", s))
        pick = check_subset(fx["states"])
        with multiprocessing.Pool(min(8, multiprocessing.cpu_count())) as pool:
            new = pool.map(solve_state, [fx["states"][i] for i in pick])
        for i, n in zip(pick, new):
            s = fx["states"][i]
            n32 = n["f64"] if n["f32"] == "=" else n["f32"]
            if not (_same(n["f64"], s["f64"]) and _same(n32, s["f32"])):
                bad.append(("roots", i, s, n))
        if bad:
            print(f"{OUT} is not what {Path(__file__).name} writes:", *bad[:5], sep="\n")
            return 1
        print(f"{OUT.name}: {len(pick)} states of {len(fx['states'])} recomputed, all current")
        return 0
    import oracle_binding as oracle
    states = build_states()
    with multiprocessing.Pool(min(8, multiprocessing.cpu_count())) as pool:
        solved = pool.map(solve_state, states, chunksize=4)
    full = []
    for s, r in zip(states, solved):
        full.append({**s, "f64": r["f64"], "f32": r["f64"] if r["f32"] == "=" else r["f32"]})
    stats, flags = oracle_alone(oracle, full)
    rows = []
    for i, (s, r) in enumerate(zip(states, solved)):
        row = {k: v for k, v in s.items() if not (k == "slope" and v == "powerlaw")}
        row.update(r)
        row["conv"] = [int(flags["f64"][i]), int(flags["f32"][i])]
        rows.append(row)
    pr = _params()
    header = {
        "generator": "tools/gen_p3_shape_roots.py --write", "equation": "tests/p3_shape_hp.py", "mpmath_digits": hp.DPS,
        "scan_spacing": 0.05, "root_tolerance": 1e-25, "eps": {"f64": 2.0 ** -52, "f32": 2.0 ** -23},
        "parameters": {k: float(v) for k, v in pr.items()}, "rtol": RTOL, "reference_budget": BUDGET,
        "strata": {k: {"n": sum(s["s"] == k for s in states), "note": v} for k, v in NOTES.items()},
        "row": ["log_lambda", "D_m", "log_N0", "df_dloglambda", "dlnDm_dloglambda", "dlogN0_dloglambda"],
        "oracle_alone": stats,
    }
    text = json.dumps({"header": header, "states": rows}, separators=(",", ":"), ensure_ascii=False)
    text = text.replace('},{"s":', '},\n{"s":').replace('"states":[', '"states":[\n')
    OUT.write_text(text + "\n")
    print(json.dumps(header["strata"], indent=1, ensure_ascii=False)[:0], json.dumps(stats, indent=1), f"{OUT}: {len(text)} bytes, {len(rows)} states")
    return 0


if __name__ == "__main__":
    sys.exit(main())
