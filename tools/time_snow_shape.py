"""HIP-event times of the snow-shape paths, alternating in one process (warm-up first; median of ROUNDS rounds of REPS calls each):
  * cmx_snow_terminal_velocity_* at 1e8 points, f32 and f64, CMX_SNOW_SHAPE_ASPR and CMX_SNOW_SHAPE_OBLATE (2 columns in, 1 out);
  * the 1-moment column step at 1e8 points (n_col × 74 levels), f32, without and with CMX_1M_SED_SNOW_OBLATE (7 in, 4 out), with the default
    options and with a non-default option set.
Prints ms per call, bytes per point and the fraction of 8 TB/s.
    python tools/time_snow_shape.py [n_points]"""
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "cloudmicrophysics.jl_amd"))
import cmx  # noqa: E402
from cmx import parameters as P, synthetic  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
ROUNDS, REPS, PEAK = 7, 10, 8e12
dev = torch.device("cuda", 0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


cases = {}
for ft, dt in (("f32", torch.float32), ("f64", torch.float64)):
    g = torch.Generator(device="cpu").manual_seed(1)
    rho = (0.3 + 1.1 * torch.rand(N, generator=g, dtype=torch.float64)).to(dt).to(dev)
    q = (10.0 ** (-10 + 8 * torch.rand(N, generator=g, dtype=torch.float64))).to(dt).to(dev)
    mp, ci = P.Microphysics1MParams(ft), P.Chen2022VelTypeIce(ft)
    for nm, sh in (("ASPR", None), ("Oblate", cmx.Oblate())):
        cases[f"snow_terminal_velocity {ft} {nm}"] = ((lambda mp=mp, ci=ci, rho=rho, q=q, sh=sh: cmx.snow_terminal_velocity(mp, ci, rho, q, sh)),
                                                      3 * rho.element_size())
n_lev = 74
n_col = N // n_lev
cols = [c.reshape(n_col, n_lev).to(dev) for c in synthetic.mp1m_state(n_col * n_lev, dtype=torch.float32, seed=3)]
inv_dz = torch.full((n_lev,), 1 / 200.0, dtype=torch.float32, device=dev)
tps = P.ThermodynamicsParameters("f32")
vel = (P.StokesRegimeVelType("f32"), P.Chen2022VelTypeRain("f32"), P.Chen2022VelTypeIce("f32"))
# default options: the unshaped step runs the default-options kernel, the shaped one the run-time-options kernel; a non-default option set runs the
# run-time-options kernel in both, which isolates what the shape itself costs
ALT = dict(cloud_ice_formation=P.TemperatureDependent(), rain_autoconversion=P.PrescribedNd())
for opt_nm, opts in (("default options", {}), ("TemperatureDependent + PrescribedNd", ALT)):
    mp1 = P.Microphysics1MParams("f32", **opts)
    for nm, sh in (("unshaped", None), ("CMX_1M_SED_SNOW_OBLATE", cmx.Oblate())):
        cases[f"1M column step f32 {opt_nm}, {nm}"] = ((lambda sh=sh, mp1=mp1: cmx.column_tendencies_sedimentation_1m(
            cmx.Instantaneous(), cmx.Microphysics1Moment(), mp1, tps, *vel, inv_dz, *cols, precip=False, snow_shape=sh)), 11 * 4)
npts = {k: (n_col * n_lev if "column" in k else N) for k in cases}
for k, (fn, _) in cases.items():            # warm-up
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in cases}
for _ in range(ROUNDS):                     # alternating: every case once per round
    for k, (fn, _) in cases.items():
        times[k].append(timed(fn))
print(f"{'case':<72} {'points':>11} {'ms':>8} {'B/point':>8} {'TB/s':>6} {'of 8 TB/s':>9}")
for k, (_, bpp) in cases.items():
    ms = statistics.median(times[k])
    tbs = npts[k] * bpp / (ms * 1e-3) / 1e12
    print(f"{k:<72} {npts[k]:>11d} {ms:>8.3f} {bpp:>8d} {tbs:>6.2f} {tbs * 1e12 / PEAK:>9.3f}")
