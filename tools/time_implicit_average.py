"""HIP-event times of the sub-stepped implicit average — cmx_sb2006_warm_rain_implicit_average_* and cmx_mp1m_implicit_average_* (include/cmx.h §19) — against
what a caller without it does, alternating in one process (warm-up first; median of ROUNDS rounds of REPS repetitions each), at 1e6 and 1e7 points, nsub 1 and
4, Δt = 30 s, f32 and f64, both schemes.  Three columns, ms per call:
  (1) the fused call: nsub substeps inside one kernel, 7 columns in, 4 out;
  (2) nsub calls of the implicit entry alone (the same state every time): the same VALU work per substep without the updates — the ratio (1)/(2) shows what
      the loop inside the kernel costs or saves; well above 1 it means lost occupancy;
  (3) the full recipe of §19 as a caller writes it today: those nsub calls plus the torch element-wise updates between them (the step, the limiter, the rates,
      the heating of T) and the final average.  The fused call has to beat this one.
States: those of tools/time_jacobian.py.  The output of the fused call and of the implicit entry is allocated once, outside the timed region; the recipe's
element-wise results allocate as torch does.
    python tools/time_implicit_average.py [--scheme sb2006|mp1m] [--ft f32|f64] [--dt SECONDS] [--nsub N …] [--fused-only] [n_points …]"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import time_jacobian as TJ  # noqa: E402  (puts the package on sys.path)
import cmx  # noqa: E402
from cmx import parameters as P  # noqa: E402

ROUNDS, REPS, DT = TJ.ROUNDS, TJ.REPS, TJ.DT
NPT = {"f32": np.float32, "f64": np.float64}


def scheme(name, ft, n, dev):
    """(fused(dt, nsub, out), implicit(cols, h, out), cols, tps) on n states"""
    if name == "sb2006":
        cols = [c.to(DT[ft]).to(dev) for c in TJ.states_sb2006(n)]
        mp, fused, implicit = P.WarmRainParams2M(ft, True), cmx.warm_rain_implicit_average_2m, cmx.warm_rain_implicit_tendencies_2m
    else:
        cols = [c.to(DT[ft]).to(dev) for c in TJ.states_mp1m(n)]
        mp, fused, implicit = P.Microphysics1MParams(ft), cmx.implicit_average_1m, cmx.implicit_tendencies_1m
    tps = P.ThermodynamicsParameters(ft)
    return (lambda dt, nsub, o: fused(mp, tps, *cols, dt, nsub, True, out=o), lambda x, h, o: implicit(mp, tps, *x, h, out=(o, None)).implicit, cols, tps)


def recipe(name, ft, implicit, cols, tps, dt, nsub, r):
    """The definition of §19 in torch over the implicit entry, limiter on (tests/implicit_average_cases.py device_recipe)."""
    FT = NPT[ft]
    h = FT(dt) / FT(nsub)
    inv_h, inv_dt, Lv, Ls = float(FT(1) / h), float(FT(1) / FT(dt)), float(FT(tps.LH_v0) / FT(tps.cp_d)), float(FT(tps.LH_s0) / FT(tps.cp_d))
    h = float(h)
    x = list(cols)
    zero = torch.zeros((), dtype=x[0].dtype, device=x[0].device)
    for _ in range(nsub):
        implicit(x, h, r)
        d = []
        for j in range(4):
            s = x[3 + j]
            lo = torch.where(s < 0, s, zero)
            sn = torch.add(s, torch.mul(r[j], h))
            sn = torch.where(sn < lo, lo, sn)
            d.append(torch.mul(torch.sub(sn, s), inv_h))
            x[3 + j] = sn
        heat = torch.mul(torch.add(d[0], d[2]), Lv)
        if name == "mp1m":
            heat = torch.add(heat, torch.mul(torch.add(d[1], d[3]), Ls))
        x[1] = torch.add(x[1], torch.mul(heat, h))
    return torch.stack([torch.mul(torch.sub(x[3 + j], cols[3 + j]), inv_dt) for j in range(4)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scheme", choices=("sb2006", "mp1m"))
    ap.add_argument("--ft", choices=("f32", "f64"))
    ap.add_argument("--dt", type=float, default=30.0)
    ap.add_argument("--nsub", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("sizes", nargs="*", type=lambda a: int(float(a)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {cmx._lib.LIB_PATH}   dt = {args.dt} s   ms per call")
    print(f"{'scheme':<7} {'type':<4} {'points':>10} {'nsub':>4} {'(1) fused':>10} {'(2) nsub x implicit':>20} {'(3) recipe':>11} {'(1)/(2)':>8} {'(1)/(3)':>8}")
    for n in args.sizes or [1_000_000, 10_000_000]:
        for name in (args.scheme,) if args.scheme else ("sb2006", "mp1m"):
            for ft in (args.ft,) if args.ft else ("f32", "f64"):
                fused, implicit, cols, tps = scheme(name, ft, n, dev)
                out, r = (torch.empty((4, n), dtype=DT[ft], device=dev) for _ in range(2))
                cases = {}
                for nsub in args.nsub:
                    h = float(NPT[ft](args.dt) / NPT[ft](nsub))
                    cases[nsub, 1] = lambda nsub=nsub: fused(args.dt, nsub, out)
                    if not args.fused_only:
                        cases[nsub, 2] = lambda nsub=nsub, h=h: [implicit(cols, h, r) for _ in range(nsub)]
                        cases[nsub, 3] = lambda nsub=nsub: recipe(name, ft, implicit, cols, tps, args.dt, nsub, r)
                for fn in cases.values():                # warm-up
                    for _ in range(2):
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in cases}
                for _ in range(ROUNDS):                 # alternating: every case once per round
                    for k, fn in cases.items():
                        times[k].append(TJ.timed(fn))
                med = {k: statistics.median(v) for k, v in times.items()}
                for nsub in args.nsub:
                    t1 = med[nsub, 1]
                    if args.fused_only:
                        print(f"{name:<7} {ft:<4} {n:>10d} {nsub:>4d} {t1:>10.3f}", flush=True)
                    else:
                        t2, t3 = med[nsub, 2], med[nsub, 3]
                        print(f"{name:<7} {ft:<4} {n:>10d} {nsub:>4d} {t1:>10.3f} {t2:>20.3f} {t3:>11.3f} {t1 / t2:>8.2f} {t1 / t3:>8.2f}", flush=True)
                del cols, out, r, cases
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
