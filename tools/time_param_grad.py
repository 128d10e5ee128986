"""HIP-event times of the parameter gradient of the SB2006 warm-rain tendencies — ONE cmx.warm_rain_param_vjp_2m call for P parameters — against the recipe a
caller had without it: per parameter two calls of the tendencies entry at θ_p ± h (h = 1e-3·|θ_p| in Float32, 1e-6·|θ_p| in Float64) and the torch
contraction Σ ḡ·(f⁺ − f⁻)/(θ⁺ − θ⁻) in float64, 2P launches in all.  Both float types and P = 1, 4, 8 alternate in ONE session on one box (every case once per
round, the median of the rounds, REPS calls per sample); states are those of tools/time_jacobian.py; the parameter structs of the recipe are built outside the
timed region, its outputs and the gradient's workspace inside it, as a caller's are.
    python tools/time_param_grad.py [n_points …]          (default 1e7)"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import time_jacobian as TJ  # noqa: E402
import cmx  # noqa: E402
from cmx import parameters as P  # noqa: E402

DT = TJ.DT
NAMES = ("SB2006_collection_kernel_coeff_kcc", "SB2006_collection_kernel_coeff_kcr", "SB2006_collection_kernel_coeff_krr",
         "SB2006_autoconversion_correcting_function_coeff_A", "SB2006_ventilation_factor_coeff_av", "SB2006_rain_evaporation_coeff_beta",
         "SB2006_raindrops_breakup_coeff_kbr", "condensation_evaporation_timescale")


def difference_recipe(ft, names, cols, gbar, tps):
    step = 1e-3 if ft == "f32" else 1e-6
    pairs = []
    for k in names:
        t = P.DEFAULT_PARAMETERS[k]
        tp, tm = t * (1 + step), t * (1 - step)
        pairs.append((P.WarmRainParams2M(P.create_toml_dict(ft, {k: tp})), P.WarmRainParams2M(P.create_toml_dict(ft, {k: tm})), tp - tm))
    scheme = cmx.Microphysics2Moment()

    def run():
        grad = []
        for plus, minus, dtheta in pairs:
            fp = torch.stack(cmx.bulk_microphysics_tendencies(scheme, plus, tps, *cols)[:4])
            fm = torch.stack(cmx.bulk_microphysics_tendencies(scheme, minus, tps, *cols)[:4])
            grad.append(((fp - fm).double() * gbar.double()).sum() / dtheta)
        return torch.stack(grad)
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("sizes", nargs="*", type=lambda a: int(float(a)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {cmx._lib.LIB_PATH}")
    for n in args.sizes or [10_000_000]:
        cases, check = {}, {}
        for ft in ("f32", "f64"):
            cols = [c.to(DT[ft]).to(dev) for c in TJ.states_sb2006(n)]
            wr, tps = P.WarmRainParams2M(ft, True), P.ThermodynamicsParameters(ft)
            g = torch.Generator(device="cpu").manual_seed(3)
            gbar = torch.stack([(torch.rand(n, generator=g, dtype=torch.float64) - 0.5).to(DT[ft]).to(dev) for _ in range(4)])
            for npar in (1, 4, 8):
                names = NAMES[:npar]
                cases[f"{ft} P={npar} param_vjp"] = lambda w=wr, t=tps, c=cols, gb=list(gbar), nm=names: cmx.warm_rain_param_vjp_2m(w, t, *c, gb, nm).grad
                cases[f"{ft} P={npar} differences"] = difference_recipe(ft, names, cols, gbar, tps)
                check[f"{ft} P={npar}"] = (cases[f"{ft} P={npar} param_vjp"], cases[f"{ft} P={npar} differences"])
        for fn in cases.values():                   # warm-up
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(TJ.ROUNDS):                  # alternating: every case once per round
            for k, fn in cases.items():
                times[k].append(TJ.timed(fn))
        med = {k: statistics.median(t) for k, t in times.items()}
        print(f"{'case':<12} {'points':>10} {'param_vjp ms':>13} {'2P launches ms':>15} {'ratio':>6} {'largest relative difference of the two gradients':>50}")
        for key, (a, b) in check.items():
            ga, gb = a().cpu(), b().cpu()
            rel = float(((ga - gb).abs() / ga.abs().clamp_min(1e-300)).max())
            print(f"{key:<12} {n:>10d} {med[key + ' param_vjp']:>13.3f} {med[key + ' differences']:>15.3f} {med[key + ' param_vjp'] / med[key + ' differences']:>6.3f} {rel:>50.2e}",
                  flush=True)


if __name__ == "__main__":
    main()
