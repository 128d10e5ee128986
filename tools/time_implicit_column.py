"""HIP-event times of the column steps with the implicit average as tendency operator — cmx_sb2006_column_implicit_average_sedimentation_* and
cmx_mp1m_column_implicit_average_sedimentation_* (include/cmx.h §20) — against what a caller without them runs, alternating in ONE process (warm-up first;
median of ROUNDS rounds of REPS repetitions each), at 1e7 points (n_lev = 64), Δt = 30 s, nsub 1 and 4, f32 and f64, both schemes.  ms per call:
  (1) the fused call: average + fall speeds + upwind sedimentation in one kernel, 7 columns in, 4 out;
  (2) the average entry alone (§19), measured THREE times per round: (2a), (2b), (2c) — their spread is the margin of the acceptance below;
  (3) the existing column entry alone, instantaneous tendencies;
  (4) the full unfused recipe: the average entry + the column entry + the tendencies entry + two torch operations (column − tendencies, + average).
Acceptance: (1) ≤ (2) + (3), within the spread max − min of (2a, 2b, 2c).  States: those of tools/time_jacobian.py, reshaped to (n_col, 64).  Outputs of the
entries are allocated once, outside the timed region, where the wrapper takes `out=`; the recipe's element-wise results allocate as torch does.
    python tools/time_implicit_column.py [--scheme sb2006|mp1m] [--ft f32|f64] [--dt SECONDS] [--nsub N …] [--n-lev L] [n_points …]"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import time_jacobian as TJ  # noqa: E402  (puts the package on sys.path)
import cmx  # noqa: E402
from cmx import parameters as P  # noqa: E402

ROUNDS, DT = TJ.ROUNDS, TJ.DT


def scheme(name, ft, n_col, n_lev, dev):
    """(fused(dt, nsub), average(dt, nsub), column(), recipe(dt, nsub)) on n_col columns of n_lev states"""
    n = n_col * n_lev
    g = torch.Generator().manual_seed(n_lev)
    inv_dz = (1.0 / (30.0 + 470.0 * torch.rand(n_lev, generator=g, dtype=torch.float64))).to(DT[ft]).to(dev)
    tps = P.ThermodynamicsParameters(ft)
    avg_out = torch.empty((4, n), dtype=DT[ft], device=dev)
    if name == "sb2006":
        cols = [c.to(DT[ft]).to(dev).reshape(n_col, n_lev) for c in TJ.states_sb2006(n)]
        flat = [c.reshape(-1) for c in cols]
        mp = P.WarmRainParams2M(ft, True)
        out_f, out_c = (cmx.ColumnTendencies2M(*[torch.empty_like(cols[0]) for _ in range(4)], None) for _ in range(2))
        out_t = cmx.WarmRainTendencies2M(*[torch.empty(n, dtype=DT[ft], device=dev) for _ in range(4)], None, None)
        fused = lambda dt, nsub: cmx.column_implicit_average_sedimentation_2m(mp, tps, inv_dz, *cols, dt, nsub, True, out=out_f)  # noqa: E731
        average = lambda dt, nsub: cmx.warm_rain_implicit_average_2m(mp, tps, *flat, dt, nsub, True, out=avg_out)  # noqa: E731
        column = lambda: cmx.column_tendencies_sedimentation(mp, tps, inv_dz, *cols, out=out_c)  # noqa: E731
        tend = lambda: cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), mp, tps, *flat, out=out_t)  # noqa: E731
    else:
        cols = [c.to(DT[ft]).to(dev).reshape(n_col, n_lev) for c in TJ.states_mp1m(n)]
        flat = [c.reshape(-1) for c in cols]
        mp = P.Microphysics1MParams(ft)
        vels = (P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft), P.Chen2022VelTypeIce(ft))
        out_t = cmx.Tendencies1M(*[torch.empty(n, dtype=DT[ft], device=dev) for _ in range(4)])
        fused = lambda dt, nsub: cmx.column_implicit_average_sedimentation_1m(mp, tps, *vels, inv_dz, *cols, dt, nsub, True, precip=False)  # noqa: E731
        average = lambda dt, nsub: cmx.implicit_average_1m(mp, tps, *flat, dt, nsub, True, out=avg_out)  # noqa: E731
        column = lambda: cmx.column_tendencies_sedimentation_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), mp, tps, *vels, inv_dz, *cols, precip=False)  # noqa: E731
        tend = lambda: cmx.bulk_microphysics_tendencies_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), mp, tps, *flat, out=out_t)  # noqa: E731

    def recipe(dt, nsub):
        a, c, t = average(dt, nsub), column(), tend()
        return [torch.add(torch.sub(c[q].reshape(-1), t[q]), a[q]) for q in range(4)]
    return fused, average, column, recipe


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scheme", choices=("sb2006", "mp1m"))
    ap.add_argument("--ft", choices=("f32", "f64"))
    ap.add_argument("--dt", type=float, default=30.0)
    ap.add_argument("--nsub", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--n-lev", type=int, default=64)
    ap.add_argument("sizes", nargs="*", type=lambda a: int(float(a)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {cmx._lib.LIB_PATH}   dt = {args.dt} s   n_lev = {args.n_lev}   ms per call")
    print(f"{'scheme':<7} {'type':<4} {'points':>10} {'nsub':>4} {'(1) fused':>10} {'(2a) avg':>9} {'(2b)':>7} {'(2c)':>7} {'(3) column':>11} {'(4) recipe':>11} "
          f"{'(2)+(3)':>8} {'spread':>7} {'(1)-(2)-(3)':>12} {'(1)/(4)':>8}")
    for n in args.sizes or [10_000_000]:
        n_col = n // args.n_lev
        for name in (args.scheme,) if args.scheme else ("sb2006", "mp1m"):
            for ft in (args.ft,) if args.ft else ("f32", "f64"):
                fused, average, column, recipe = scheme(name, ft, n_col, args.n_lev, dev)
                cases = {}
                for nsub in args.nsub:
                    cases[nsub, "1"] = lambda nsub=nsub: fused(args.dt, nsub)
                    for rep in "abc":
                        cases[nsub, "2" + rep] = lambda nsub=nsub: average(args.dt, nsub)
                    cases[nsub, "4"] = lambda nsub=nsub: recipe(args.dt, nsub)
                cases[0, "3"] = column
                for fn in cases.values():                # warm-up
                    for _ in range(2):
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in cases}
                for _ in range(ROUNDS):                 # alternating: every case once per round
                    for k, fn in cases.items():
                        times[k].append(TJ.timed(fn))
                med = {k: statistics.median(v) for k, v in times.items()}
                t3 = med[0, "3"]
                for nsub in args.nsub:
                    t1, t2, t4 = med[nsub, "1"], [med[nsub, "2" + rep] for rep in "abc"], med[nsub, "4"]
                    mid = statistics.median(t2)
                    print(f"{name:<7} {ft:<4} {n_col * args.n_lev:>10d} {nsub:>4d} {t1:>10.3f} {t2[0]:>9.3f} {t2[1]:>7.3f} {t2[2]:>7.3f} {t3:>11.3f} {t4:>11.3f} "
                          f"{mid + t3:>8.3f} {max(t2) - min(t2):>7.3f} {t1 - mid - t3:>12.3f} {t1 / t4:>8.2f}", flush=True)
                del fused, average, column, recipe, cases
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
