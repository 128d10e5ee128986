"""HIP-event times of cmx_mp1m_jacobian_* against what a caller without it does, alternating in one process (warm-up first; median of ROUNDS rounds of
REPS repetitions each), at 1e6 and 1e7 points, f32 and f64:
  * ONE Jacobian call: the full 4 × 6 Jacobian with the four tendencies (7 columns in, 28 out: 140 B/point in f32);
  * the same without the tendencies (7 in, 24 out), and the four-species block wrt = (q_lcl, q_icl, q_rai, q_sno) an implicit step of the species solves;
  * central differences over the six inputs plus the primal: 13 calls of cmx_mp1m_tendencies_* (7 in, 4 out each: 13 × 44 B/point in f32) — the launches
    only; forming the 12 perturbed columns and the 24 quotients is left out, in the caller's favour.
Inputs: states with all four species present on both sides of T_freeze (the regime of the Jacobian tests), drawn on the host.  Outputs are allocated once,
outside the timed region.  Prints ms per Jacobian, the ratio to the 13 launches, bytes per point and the fraction of 8 TB/s on the algorithmic bytes.
A library built with other tangents per pass (-DCMX_JAC1M_K_F32=…, -DCMX_JAC1M_K_F64=…) is timed by pointing CMX_LIB at it.
    python tools/time_mp1m_jacobian.py [--ft f32|f64] [n_points …]"""
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "cloudmicrophysics.jl_amd"))
import cmx  # noqa: E402
from cmx import parameters as P  # noqa: E402

args = sys.argv[1:]
FTS = ("f32", "f64")
if "--ft" in args:
    k = args.index("--ft")
    FTS = (args[k + 1],)
    del args[k:k + 2]
SIZES = [int(float(a)) for a in args] or [1_000_000, 10_000_000]
ROUNDS, REPS, PEAK = 7, 5, 8e12
DT = {"f32": torch.float32, "f64": torch.float64}
BASE = "13 tendencies launches (central differences + primal)"
dev = torch.device("cuda", 0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def states(n, dt):
    g = torch.Generator(device="cpu").manual_seed(11)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)  # noqa: E731
    rho, T = u(0.4, 1.2), u(235.0, 300.0)
    q_lcl, q_icl = 10.0 ** u(-6.0, -3.0), 10.0 ** u(-6.0, -3.0)
    q_rai, q_sno = 10.0 ** u(-6.0, -2.7), 10.0 ** u(-6.0, -2.7)
    q_sat = 611.657 * torch.exp(17.5 * (T - 273.16) / (T - 32.0)) / (rho * 461.5 * T)      # Magnus-type: only the regime matters here
    q_tot = q_lcl + q_icl + q_rai + q_sno + q_sat * u(0.5, 1.05)
    return [c.to(dt).to(dev) for c in (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno)]


print(f"library: {cmx._lib.LIB_PATH}")
print(f"{'case':<62} {'points':>10} {'ms':>8} {'vs 13 launches':>14} {'B/point':>8} {'TB/s':>6} {'of 8 TB/s':>9}")
for n in SIZES:
    cases = {}
    for ft in FTS:
        dt = DT[ft]
        cols = states(n, dt)
        mp, tps, e = P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft), cols[0].element_size()
        jac, tend = torch.empty((4, 6, n), dtype=dt, device=dev), torch.empty((4, n), dtype=dt, device=dev)
        jac4 = torch.empty((4, 4, n), dtype=dt, device=dev)
        out = cmx.Tendencies1M(*[torch.empty(n, dtype=dt, device=dev) for _ in range(4)])
        mode, sch = cmx.Instantaneous(), cmx.Microphysics1Moment()

        def full(mp=mp, tps=tps, cols=cols, jac=jac, tend=tend):
            cmx.jacobian_1m(mp, tps, *cols, with_tendencies=True, out=(jac, tend))

        def no_tend(mp=mp, tps=tps, cols=cols, jac=jac):
            cmx.jacobian_1m(mp, tps, *cols, out=(jac, None))

        def species(mp=mp, tps=tps, cols=cols, jac4=jac4):
            cmx.jacobian_1m(mp, tps, *cols, wrt=("q_lcl", "q_icl", "q_rai", "q_sno"), out=(jac4, None))

        def differences(mp=mp, tps=tps, cols=cols, out=out, mode=mode, sch=sch):
            for _ in range(13):
                cmx.bulk_microphysics_tendencies_1m(mode, sch, mp, tps, *cols, out=out)
        cases[f"{ft} jacobian 4x6 + tendencies (one call)"] = (full, 35 * e, ft)
        cases[f"{ft} jacobian 4x6"] = (no_tend, 31 * e, ft)
        cases[f"{ft} jacobian 4x4 (q_lcl, q_icl, q_rai, q_sno)"] = (species, 23 * e, ft)
        cases[f"{ft} {BASE}"] = (differences, 13 * 11 * e, ft)
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
        base = med[f"{ft} {BASE}"]
        tbs = n * bpp / (med[k] * 1e-3) / 1e12
        print(f"{k:<62} {n:>10d} {med[k]:>8.3f} {med[k] / base:>14.3f} {bpp:>8d} {tbs:>6.2f} {tbs * 1e12 / PEAK:>9.3f}", flush=True)
