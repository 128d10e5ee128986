"""HIP-event times of the 2M + P3 column step with backward-Euler sedimentation — cmx_mp2m_p3_column_implicit_sedimentation_* (include/cmx.h §24) — against the
explicit step (9b), cmx_mp2m_p3_column_tendencies_sedimentation_*, alternating in ONE process (warm-up first; median of ROUNDS rounds, every case once per
round), at 1e6 points (n_lev = 64), Δt = 300 s, Float32 and Float64, quadrature order 16, the mixed-phase states of tests/p3_column_ref.py.  ms per call:
  (a)  the new entry: products → shape + fall speeds → tendencies → the top-down recurrence kernel;
  (b1), (b2) the (9b) entry, measured TWICE per round: their difference is the noise floor of (a)/(b).
Steps 1 and 2 are the same launches in both, so (a) − (b) is the difference between the two sedimentation kernels.  Outputs are allocated once, outside the
timed region.  Before timing: at Δt = 0 the new entry returns the (9b) entry's values (log λ and the ice speeds bit for bit) at the size that is timed.
    python tools/time_p3_implicit_column.py [--ft f32|f64] [--dt SECONDS] [--n-lev L] [--cloud] [--vel sb|chen] [n_points …]"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO / "cloudmicrophysics.jl_amd", REPO / "tests"):
    sys.path.insert(0, str(p))
import cmx  # noqa: E402
from cmx import parameters as P  # noqa: E402
import p3_column_ref as R  # noqa: E402

ROUNDS = 9
DT = {"f32": torch.float32, "f64": torch.float64}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def make(ft, n_col, n_lev, cloud, vel, dev):
    """(implicit(dt), explicit()) on n_col columns of n_lev states, each with outputs of its own"""
    s = R.states(n_col, n_lev, seed=19, f32_safe=(ft == "f32"))
    d = {k: torch.from_numpy(v).to(DT[ft]).to(dev) for k, v in s.items()}
    dz = torch.from_numpy(R.inv_dz(n_lev, seed=1)).to(DT[ft]).to(dev)
    mp, tps = P.Microphysics2MParams(ft, with_ice=True), P.ThermodynamicsParameters(ft)
    cols = [d[k] for k in R.IN_NAMES]
    kw = dict(vel=cmx.SB2006VelType if vel == "sb" else cmx.Chen2022VelTypeRain, cloud_vel=P.StokesRegimeVelType(ft) if cloud else None)
    mk = lambda: cmx.ColumnTendencies2MP3(*[torch.empty_like(d["rho"]) for _ in range(11)], *[torch.empty(n_col, dtype=DT[ft], device=dev) for _ in range(2)])  # noqa: E731
    out_a, out_b = mk(), mk()
    implicit = lambda dt: cmx.column_implicit_sedimentation_2m_p3(mp, tps, dz, *cols, dt, out=out_a, **kw)  # noqa: E731
    explicit = lambda: cmx.column_tendencies_sedimentation_2m_p3(mp, tps, dz, *cols, out=out_b, **kw)  # noqa: E731
    return implicit, explicit


def same_values(a, b):
    return bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--ft", choices=("f32", "f64"))
    ap.add_argument("--dt", type=float, default=300.0)
    ap.add_argument("--n-lev", type=int, default=64)
    ap.add_argument("--cloud", action="store_true", help="with cloud sedimentation (eight falling species instead of six)")
    ap.add_argument("--vel", choices=("sb", "chen"), default="sb")
    ap.add_argument("sizes", nargs="*", type=lambda a: int(float(a)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {cmx._lib.LIB_PATH}   dt = {args.dt} s   n_lev = {args.n_lev}   cloud_vel = {args.cloud}   rain speeds: {args.vel}   "
          f"median of {ROUNDS} alternating rounds, ms per call")
    print(f"{'type':<4} {'points':>10} {'(a) implicit':>12} {'(b1) (9b)':>10} {'(b2)':>8} {'(a)/(b)':>8} {'(b1)/(b2)':>9} {'(a)-(b)':>8} {'spread of (a)':>16}  dt = 0 check")
    for n in args.sizes or [1_000_000]:
        n_col = n // args.n_lev
        for ft in (args.ft,) if args.ft else ("f32", "f64"):
            implicit, explicit = make(ft, n_col, args.n_lev, args.cloud, args.vel, dev)
            got, want = implicit(0.0), explicit()      # warm-up, and the comparison of the two results
            torch.cuda.synchronize()
            agree = all(same_values(x, y) for x, y in zip(got, want)) and all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(got[8:11], want[8:11]))
            cases = {"b1": explicit, "a": lambda: implicit(args.dt), "b2": explicit}
            for fn in cases.values():
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in cases}
            for _ in range(ROUNDS):                     # alternating: every case once per round
                for k, fn in cases.items():
                    times[k].append(timed(fn))
            ta, tb1, tb2 = (statistics.median(times[k]) for k in ("a", "b1", "b2"))
            tb = 0.5 * (tb1 + tb2)
            print(f"{ft:<4} {n_col * args.n_lev:>10d} {ta:>12.3f} {tb1:>10.3f} {tb2:>8.3f} {ta / tb:>8.3f} {tb1 / tb2:>9.3f} {ta - tb:>8.3f} "
                  f"{min(times['a']):>7.3f}-{max(times['a']):<8.3f}  {'same values' if agree else 'DIFFERENT'}", flush=True)
            del implicit, explicit, cases, got, want
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
