"""HIP-event times of the column steps with backward-Euler sedimentation — cmx_sb2006_column_implicit_step_* and cmx_mp1m_column_implicit_step_*
(include/cmx.h §21) — against the explicit step of §20 and against what a caller without them runs, alternating in ONE process (warm-up first; median of ROUNDS
rounds, every case once per round), at 1e7 points (n_lev = 64), Δt = 300 s, nsub 1 and 2, f32 and f64, both schemes.  ms per call:
  (a) the new entry: average + fall speeds + the top-down recurrence in one kernel, 7 columns in, 4 out;
  (b) the §20 entry, measured TWICE per round — (b1), (b2): their difference is the noise floor of (a)/(b) — : the cost of making sedimentation implicit;
  (c) the recipe a user has without (a): the average entry, the velocity entries and a level-by-level torch loop over the columns.
States: those of tools/time_jacobian.py, reshaped to (n_col, 64).  Outputs of the entries are allocated once, outside the timed region, where the wrapper takes
`out=`; the recipe's element-wise results allocate as torch does.
    python tools/time_implicit_step.py [--scheme sb2006|mp1m] [--ft f32|f64] [--dt SECONDS] [--nsub N …] [--n-lev L] [n_points …]"""
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
    """(implicit(dt, nsub), explicit(dt, nsub), recipe(dt, nsub)) on n_col columns of n_lev states"""
    n = n_col * n_lev
    g = torch.Generator().manual_seed(n_lev)
    inv_dz = (1.0 / (30.0 + 470.0 * torch.rand(n_lev, generator=g, dtype=torch.float64))).to(DT[ft]).to(dev)
    tps = P.ThermodynamicsParameters(ft)
    avg_out = torch.empty((4, n), dtype=DT[ft], device=dev)
    if name == "sb2006":
        cols = [c.to(DT[ft]).to(dev).reshape(n_col, n_lev) for c in TJ.states_sb2006(n)]
        flat = [c.reshape(-1) for c in cols]
        mp = P.WarmRainParams2M(ft, True)
        out_a, out_b = (cmx.ColumnTendencies2M(*[torch.empty_like(cols[0]) for _ in range(4)], None) for _ in range(2))
        out_t = cmx.WarmRainTendencies2M(*[torch.empty(n, dtype=DT[ft], device=dev) for _ in range(6)])
        implicit = lambda dt, nsub: cmx.column_implicit_step_2m(mp, tps, inv_dz, *cols, dt, nsub, True, out=out_a)  # noqa: E731
        explicit = lambda dt, nsub: cmx.column_implicit_average_sedimentation_2m(mp, tps, inv_dz, *cols, dt, nsub, True, out=out_b)  # noqa: E731
        average = lambda dt, nsub: cmx.warm_rain_implicit_average_2m(mp, tps, *flat, dt, nsub, True, out=avg_out)  # noqa: E731

        def speeds():      # the rain velocities of the tendencies entry; the cloud does not fall in this configuration
            t = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), mp, tps, *flat, vel=cmx.SB2006VelType, out=out_t)
            return [None, None, t.vt_rai_m.reshape(n_col, n_lev), t.vt_rai_n.reshape(n_col, n_lev)]
    else:
        cols = [c.to(DT[ft]).to(dev).reshape(n_col, n_lev) for c in TJ.states_mp1m(n)]
        flat = [c.reshape(-1) for c in cols]
        mp = P.Microphysics1MParams(ft)
        vels = (P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft), P.Chen2022VelTypeIce(ft))
        implicit = lambda dt, nsub: cmx.column_implicit_step_1m(mp, tps, *vels, inv_dz, *cols, dt, nsub, True, precip=False)  # noqa: E731
        explicit = lambda dt, nsub: cmx.column_implicit_average_sedimentation_1m(mp, tps, *vels, inv_dz, *cols, dt, nsub, True, precip=False)  # noqa: E731
        average = lambda dt, nsub: cmx.implicit_average_1m(mp, tps, *flat, dt, nsub, True, out=avg_out)  # noqa: E731
        speeds = lambda: [w.reshape(n_col, n_lev) for w in cmx.sedimentation_velocities(mp, *vels, flat[0], *flat[3:])]  # noqa: E731

    def recipe(dt, nsub):
        """§21 in torch: the element-wise part over whole (n_col, n_lev) tensors, the recurrence level by level from the top."""
        a = average(dt, nsub).reshape(4, n_col, n_lev)
        rho = cols[0].clamp(min=0)
        gk = inv_dz / rho
        out = []
        for q, w in enumerate(speeds()):
            if w is None:
                out.append(a[q])
                continue
            F = rho * cols[3 + q].clamp(min=0) * w
            tau = dt * w
            c = tau * inv_dz
            r = 1.0 / (1.0 + c)
            A, G = c * r, torch.addcmul(F, tau * rho, a[q]) * r      # G starts as B
            for k in range(n_lev - 2, -1, -1):
                G[:, k].addcmul_(A[:, k], G[:, k + 1])
            up = torch.zeros_like(G)
            up[:, :-1] = G[:, 1:]
            out.append(((up - F) * gk + a[q]) * r)
        return out
    return implicit, explicit, recipe


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scheme", choices=("sb2006", "mp1m"))
    ap.add_argument("--ft", choices=("f32", "f64"))
    ap.add_argument("--dt", type=float, default=300.0)
    ap.add_argument("--nsub", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--n-lev", type=int, default=64)
    ap.add_argument("sizes", nargs="*", type=lambda a: int(float(a)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {cmx._lib.LIB_PATH}   dt = {args.dt} s   n_lev = {args.n_lev}   ms per call")
    print(f"{'scheme':<7} {'type':<4} {'points':>10} {'nsub':>4} {'(a) implicit':>12} {'(b1) §20':>9} {'(b2)':>8} {'(c) recipe':>11} {'(a)/(b)':>8} {'(b1)/(b2)':>9} {'(c)/(a)':>8}")
    for n in args.sizes or [10_000_000]:
        n_col = n // args.n_lev
        for name in (args.scheme,) if args.scheme else ("sb2006", "mp1m"):
            for ft in (args.ft,) if args.ft else ("f32", "f64"):
                implicit, explicit, recipe = scheme(name, ft, n_col, args.n_lev, dev)
                cases = {}
                for nsub in args.nsub:
                    cases[nsub, "b1"] = lambda nsub=nsub: explicit(args.dt, nsub)
                    cases[nsub, "a"] = lambda nsub=nsub: implicit(args.dt, nsub)
                    cases[nsub, "b2"] = lambda nsub=nsub: explicit(args.dt, nsub)
                    cases[nsub, "c"] = lambda nsub=nsub: recipe(args.dt, nsub)
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
                    ta, tb1, tb2, tc = (med[nsub, k] for k in ("a", "b1", "b2", "c"))
                    tb = 0.5 * (tb1 + tb2)
                    print(f"{name:<7} {ft:<4} {n_col * args.n_lev:>10d} {nsub:>4d} {ta:>12.3f} {tb1:>9.3f} {tb2:>8.3f} {tc:>11.3f} {ta / tb:>8.3f} {tb1 / tb2:>9.3f} "
                          f"{tc / ta:>8.2f}", flush=True)
                del implicit, explicit, recipe, cases
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
