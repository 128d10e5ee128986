#!/usr/bin/env python3
"""The Float32 bound of the parcel-run GPU test, from the reference restatement alone.

A forward-Euler parcel integration amplifies rounding (ABIFM_J = 10^(m Δa_w + c) with m ≈ 54, hundreds of steps), so the project's plain 1e-3 does not
hold for a Float32 run and cannot be fixed in advance.  For every ensemble of tests/parcel_cases.py this tool runs tests/parcel_ref.py — the NumPy
restatement of the reference — once in np.float32 and once in np.float64 on the same Float32-rounded inputs and records, per variable, the largest
difference on the scales of the test (S_l, p, T on their own magnitude; q on q_tot; N on N_aer + N_liq + N_ice), parcels inside the gate mask left
out.  The GPU test allows the device four times that spread (parcel_cases.SPREAD_FACTOR: hardware exp / log are within a few ulp where NumPy's are
within one, and both perturb the same recurrence).  The code under test takes no part in producing the numbers.

    python tools/gen_parcel_spread.py            # rewrites tests/golden/parcel_f32_spread.json
"""
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
for p in (REPO / "cloudmicrophysics.jl_amd", REPO / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import parcel_cases as PC  # noqa: E402
import parcel_ref as R  # noqa: E402


def spread_of(case, step_counts):
    """{str(steps): {variable: max scaled |Float32 − Float64| of the restatement}} for one ensemble."""
    cfg = PC.RUN_CASES[case]
    _, prm = PC.build("f64", **cfg["kw"])
    Y0, w = PC.run_ensemble(case, prm)
    Y32, w32 = [y.astype(np.float32) for y in Y0], w.astype(np.float32)
    opt = PC.ref_options(cfg["kw"])
    out = {}
    for steps in step_counts:
        r64 = R.run(np.float64, prm, opt, Y32, w32, steps, margin=PC.MARGIN["f32"])
        r32 = R.run(np.float32, prm, opt, Y32, w32, steps)
        keep = ~r64["near_gate"]
        err = PC.scaled_run_error(r32["final"], r64["final"], [y.astype(np.float64) for y in Y32])[:, keep]
        if not np.all(np.isfinite(err)):
            raise SystemExit(f"{case}: the Float32 restatement is not finite at {steps} steps")
        out[str(steps)] = {name: float(np.max(err[j])) for j, name in enumerate(R.STATE)}
    return out


def main():
    result = {}
    for case in PC.F32_RUN_CASES:
        cfg = PC.RUN_CASES[case]
        counts = sorted({100, cfg["steps32"]})
        result[case] = spread_of(case, counts)
        for steps, row in result[case].items():
            print(case, steps, " ".join(f"{k}={v:.2e}" for k, v in row.items()))
    PC.SPREAD_FILE.write_text(json.dumps(result, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
