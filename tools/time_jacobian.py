"""HIP-event times of a Jacobian entry — cmx_sb2006_warm_rain_jacobian_* (--scheme sb2006) or cmx_mp1m_jacobian_* (--scheme mp1m) — against what a
caller without it does, alternating in one process (warm-up first; median of ROUNDS rounds of REPS repetitions each), at 1e6 and 1e7 points, f32 and f64:
  * ONE Jacobian call: the full 4 × 6 Jacobian with the four tendencies (7 columns in, 28 out: 140 B/point in f32);
  * the same without the tendencies (7 in, 24 out), and a selection of columns: sb2006 wrt = (q_lcl, q_rai, n_rai) (one pass in Float32), mp1m the
    four-species block wrt = (q_lcl, q_icl, q_rai, q_sno) an implicit step of the species solves;
  * central differences over the six inputs plus the primal: 13 calls of the scheme's tendencies entry (7 in, 4 out each: 13 × 44 B/point in f32) — the
    launches only; forming the 12 perturbed columns and the 24 quotients is left out, in the caller's favour.
Inputs: the regime of the scheme's Jacobian tests (all four species present; mp1m: both sides of T_freeze), drawn on the host.  Outputs are allocated
once, outside the timed region.  Prints ms per Jacobian, the ratio to the 13 launches, bytes per point and the fraction of 8 TB/s on the algorithmic bytes.
A library built with other tangents per pass (-DCMX_JAC_K_F32=…, -DCMX_JAC1M_K_F64=…, …) is timed by pointing CMX_LIB at it.
    python tools/time_jacobian.py --scheme sb2006|mp1m [--ft f32|f64] [n_points …]"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "cloudmicrophysics.jl_amd"))
import cmx  # noqa: E402
from cmx import parameters as P  # noqa: E402

ROUNDS, REPS, PEAK = 7, 5, 8e12
DT = {"f32": torch.float32, "f64": torch.float64}
BASE = "13 tendencies launches (central differences + primal)"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def _q_sat(T, rho):
    return 611.657 * torch.exp(17.5 * (T - 273.16) / (T - 32.0)) / (rho * 461.5 * T)      # Magnus-type: only the regime matters here


def states_sb2006(n):
    g = torch.Generator(device="cpu").manual_seed(7)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)  # noqa: E731
    rho, T = u(0.6, 1.2), u(275.0, 300.0)
    q_lcl, q_rai = 10.0 ** u(-5.0, -2.7), 10.0 ** u(-6.0, -2.7)
    n_lcl, n_rai = q_lcl / 10.0 ** u(-12.2, -10.0), q_rai / 10.0 ** u(-9.5, -6.2)
    q_tot = q_lcl + q_rai + _q_sat(T, rho) * u(0.5, 1.05)
    return rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai


def states_mp1m(n):
    g = torch.Generator(device="cpu").manual_seed(11)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)  # noqa: E731
    rho, T = u(0.4, 1.2), u(235.0, 300.0)
    q_lcl, q_icl = 10.0 ** u(-6.0, -3.0), 10.0 ** u(-6.0, -3.0)
    q_rai, q_sno = 10.0 ** u(-6.0, -2.7), 10.0 ** u(-6.0, -2.7)
    q_tot = q_lcl + q_icl + q_rai + q_sno + _q_sat(T, rho) * u(0.5, 1.05)
    return rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno


def scheme_sb2006(ft, n, dev):
    """(jacobian(**kw), one tendencies launch, the selection of columns) on n states"""
    cols = [c.to(DT[ft]).to(dev) for c in states_sb2006(n)]
    wr, tps, sch = P.WarmRainParams2M(ft, True), P.ThermodynamicsParameters(ft), cmx.Microphysics2Moment()
    out = cmx.WarmRainTendencies2M(*[torch.empty(n, dtype=DT[ft], device=dev) for _ in range(4)], None, None)
    return (lambda **kw: cmx.warm_rain_jacobian_2m(wr, tps, *cols, **kw), lambda: cmx.bulk_microphysics_tendencies(sch, wr, tps, *cols, out=out),
            ("q_lcl", "q_rai", "n_rai"))


def scheme_mp1m(ft, n, dev):
    cols = [c.to(DT[ft]).to(dev) for c in states_mp1m(n)]
    mp, tps, mode, sch = P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft), cmx.Instantaneous(), cmx.Microphysics1Moment()
    out = cmx.Tendencies1M(*[torch.empty(n, dtype=DT[ft], device=dev) for _ in range(4)])
    return (lambda **kw: cmx.jacobian_1m(mp, tps, *cols, **kw), lambda: cmx.bulk_microphysics_tendencies_1m(mode, sch, mp, tps, *cols, out=out),
            ("q_lcl", "q_icl", "q_rai", "q_sno"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scheme", required=True, choices=("sb2006", "mp1m"))
    ap.add_argument("--ft", choices=("f32", "f64"))
    ap.add_argument("sizes", nargs="*", type=lambda a: int(float(a)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {cmx._lib.LIB_PATH}")
    print(f"{'case':<62} {'points':>10} {'ms':>8} {'vs 13 launches':>14} {'B/point':>8} {'TB/s':>6} {'of 8 TB/s':>9}")
    for n in args.sizes or [1_000_000, 10_000_000]:
        cases = {}
        for ft in (args.ft,) if args.ft else ("f32", "f64"):
            jacobian, tendencies, sel = {"sb2006": scheme_sb2006, "mp1m": scheme_mp1m}[args.scheme](ft, n, dev)
            e = torch.empty(0, dtype=DT[ft]).element_size()
            jac, tend = torch.empty((4, 6, n), dtype=DT[ft], device=dev), torch.empty((4, n), dtype=DT[ft], device=dev)
            jsel = torch.empty((4, len(sel), n), dtype=DT[ft], device=dev)
            cases[f"{ft} jacobian 4x6 + tendencies (one call)"] = (lambda j=jacobian, o=(jac, tend): j(with_tendencies=True, out=o), 35 * e, ft)
            cases[f"{ft} jacobian 4x6"] = (lambda j=jacobian, o=(jac, None): j(out=o), 31 * e, ft)
            cases[f"{ft} jacobian 4x{len(sel)} ({', '.join(sel)})"] = (lambda j=jacobian, o=(jsel, None), w=sel: j(wrt=w, out=o), (7 + 4 * len(sel)) * e, ft)
            cases[f"{ft} {BASE}"] = (lambda t=tendencies: [t() for _ in range(13)], 13 * 11 * e, ft)
        for fn, _, _ in cases.values():             # warm-up
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(ROUNDS):                     # alternating: every case once per round
            for k, (fn, _, _) in cases.items():
                times[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, (_, bpp, ft) in cases.items():
            tbs = n * bpp / (med[k] * 1e-3) / 1e12
            print(f"{k:<62} {n:>10d} {med[k]:>8.3f} {med[k] / med[f'{ft} {BASE}']:>14.3f} {bpp:>8d} {tbs:>6.2f} {tbs * 1e12 / PEAK:>9.3f}", flush=True)


if __name__ == "__main__":
    main()
