"""HIP-event times of the fused linearly implicit tendencies — cmx_sb2006_warm_rain_implicit_tendencies_* (--scheme sb2006) or cmx_mp1m_implicit_tendencies_*
(--scheme mp1m) — against what a caller without them does, alternating in one process (warm-up first; median of ROUNDS rounds of REPS repetitions each), at
1e6 and 1e7 points, f32 and f64:
  * the fused entry: r = (I − Δt J)⁻¹ f, 7 columns in, 4 out (44 B/point in f32);
  * the tendencies entry alone (7 in, 4 out): the floor — the fused entry moves the same bytes;
  * the recipe of INTEGRATION.md (v) / (vi): the Jacobian entry with the four species and the tendencies (7 in, 20 out), `A = I − Δt·jac.permute(2, 0, 1)`
    and `torch.linalg.solve(A, tendencies.T)` over all points (20 in again, 4 out, and a batched LU of n 4 × 4 matrices); the same without the solve is
    printed too, so that the share of the Jacobian entry is visible.  No scaling before the solve, in the recipe's favour.
States: those of tools/time_jacobian.py.  Outputs of the entries are allocated once, outside the timed region; the recipe's A and its solve allocate as
torch does.  Prints ms per call and the ratio to the recipe.  A library built with other tangents per pass (-DCMX_IMPLICIT_K_F32=…, -DCMX_IMPLICIT_K_F64=…)
is timed by pointing CMX_LIB at it; --fused-only times the fused entry alone (for such a comparison).
    python tools/time_implicit.py --scheme sb2006|mp1m [--ft f32|f64] [--dt SECONDS] [--fused-only] [n_points …]"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import time_jacobian as TJ  # noqa: E402  (puts the package on sys.path)
import cmx  # noqa: E402
from cmx import parameters as P  # noqa: E402

ROUNDS, REPS, DT = TJ.ROUNDS, TJ.REPS, TJ.DT
FUSED, FLOOR, RECIPE, JAC = "fused implicit tendencies", "tendencies entry alone", "recipe: jacobian 4x4 + tendencies, torch.linalg.solve", "  of which the jacobian entry"


def scheme_sb2006(ft, n, dev):
    """(fused(dt, out), jacobian(out), one tendencies launch, the species) on n states"""
    cols = [c.to(DT[ft]).to(dev) for c in TJ.states_sb2006(n)]
    wr, tps, sch = P.WarmRainParams2M(ft, True), P.ThermodynamicsParameters(ft), cmx.Microphysics2Moment()
    out = cmx.WarmRainTendencies2M(*[torch.empty(n, dtype=DT[ft], device=dev) for _ in range(4)], None, None)
    sel = ("q_lcl", "n_lcl", "q_rai", "n_rai")
    return (lambda dt, o: cmx.warm_rain_implicit_tendencies_2m(wr, tps, *cols, dt, out=o),
            lambda o: cmx.warm_rain_jacobian_2m(wr, tps, *cols, wrt=sel, with_tendencies=True, out=o),
            lambda: cmx.bulk_microphysics_tendencies(sch, wr, tps, *cols, out=out))


def scheme_mp1m(ft, n, dev):
    cols = [c.to(DT[ft]).to(dev) for c in TJ.states_mp1m(n)]
    mp, tps, mode, sch = P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft), cmx.Instantaneous(), cmx.Microphysics1Moment()
    out = cmx.Tendencies1M(*[torch.empty(n, dtype=DT[ft], device=dev) for _ in range(4)])
    sel = ("q_lcl", "q_icl", "q_rai", "q_sno")
    return (lambda dt, o: cmx.implicit_tendencies_1m(mp, tps, *cols, dt, out=o),
            lambda o: cmx.jacobian_1m(mp, tps, *cols, wrt=sel, with_tendencies=True, out=o),
            lambda: cmx.bulk_microphysics_tendencies_1m(mode, sch, mp, tps, *cols, out=out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scheme", required=True, choices=("sb2006", "mp1m"))
    ap.add_argument("--ft", choices=("f32", "f64"))
    ap.add_argument("--dt", type=float, default=30.0)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("sizes", nargs="*", type=lambda a: int(float(a)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {cmx._lib.LIB_PATH}   dt = {args.dt} s")
    print(f"{'case':<64} {'points':>10} {'ms':>9} {'vs recipe':>10}")
    for n in args.sizes or [1_000_000, 10_000_000]:
        cases = {}
        for ft in (args.ft,) if args.ft else ("f32", "f64"):
            fused, jacobian, tendencies = {"sb2006": scheme_sb2006, "mp1m": scheme_mp1m}[args.scheme](ft, n, dev)
            r = torch.empty((4, n), dtype=DT[ft], device=dev)
            cases[f"{ft} {FUSED}"] = (lambda f=fused, o=(r, None): f(args.dt, o), ft)
            if args.fused_only:
                continue
            jac, tend = torch.empty((4, 4, n), dtype=DT[ft], device=dev), torch.empty((4, n), dtype=DT[ft], device=dev)
            eye = torch.eye(4, dtype=DT[ft], device=dev)

            def recipe(j=jacobian, o=(jac, tend), eye=eye):
                j(o)
                return torch.linalg.solve(eye - args.dt * o[0].permute(2, 0, 1), o[1].T)
            cases[f"{ft} {FLOOR}"] = (tendencies, ft)
            cases[f"{ft} {RECIPE}"] = (recipe, ft)
            cases[f"{ft} {JAC}"] = (lambda j=jacobian, o=(jac, tend): j(o), ft)
        for fn, _ in cases.values():                # warm-up
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(ROUNDS):                     # alternating: every case once per round
            for k, (fn, _) in cases.items():
                times[k].append(TJ.timed(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, (_, ft) in cases.items():
            ratio = f"{med[k] / med[f'{ft} {RECIPE}']:>10.3f}" if not args.fused_only else f"{'':>10}"
            print(f"{k:<64} {n:>10d} {med[k]:>9.3f} {ratio}", flush=True)


if __name__ == "__main__":
    main()
