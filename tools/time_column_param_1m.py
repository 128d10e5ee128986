"""HIP-event times of the derivatives of the 1-moment column step with respect to the PARAMETERS — cmx_mp1m_column_param_jvp_* for KP directions (one wide
launch) and for 16, cmx_mp1m_column_param_vjp_* for the gradient with respect to 16 names — beside the primal column entry of the SAME build on the same box
and beside 2·ndir primal calls: what central differences cost, the only recipe without these entries.  Columns of 64 levels, states of tools/time_jacobian.py,
both float types, default parameters; every output is allocated once, outside the timed region, and the entries are called through the raw ABI.  All cases
alternate in one session (every case once per round, the median of the rounds); the session is repeated `--runs` times.  With `--primal-only` only the primal
entry is timed: run so with CMX_LIB pointing at another build's library, in alternating processes, for a baseline.
    python tools/time_column_param_1m.py [--runs 3] [--levels 64] [--primal-only] [n_points …]          (default 1e7)"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import time_jacobian as TJ  # noqa: E402
import cmx  # noqa: E402
from cmx import _abi, _lib  # noqa: E402
from cmx import parameters as P  # noqa: E402

DT = TJ.DT
KP = {"f32": 4, "f64": 2}      # csrc/cmx_mp1m_column_param.hpp kCol1mParamK
NAMES = ("Chen2022_table_B1_ai[0]", "Chen2022_table_B1_q_coeff", "Chen2022_table_B3_As[0]", "Chen2022_table_B5_Al[0]", "Chen2022_table_B5_Cl[1]",
         "snow_aspect_ratio", "snow_apparent_density", "cloud_ice_apparent_density", "cloud_liquid_sedimentation_number_concentration",
         "gravitational_acceleration", "density_liquid_water", "kinematic_viscosity_of_air", "rain_drop_size_distribution_coefficient_n0",
         "snow_flake_size_distribution_coefficient_mu", "rain_autoconversion_timescale", "latent_heat_vaporization_at_reference")


def cases_of(ft, n_col, n_lev, dev, primal_only):
    n = n_col * n_lev
    cols = [c.to(DT[ft]).to(dev).reshape(n_col, n_lev).contiguous() for c in TJ.states_mp1m(n)]
    mp, tps, stokes, cr, ci = structs = (P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft), P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft),
                                         P.Chen2022VelTypeIce(ft))
    fam = _abi.F32 if ft == "f32" else _abi.F64
    inv_dz = (1.0 / torch.linspace(40.0, 400.0, n_lev, dtype=torch.float64)).to(DT[ft]).to(dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda shape: (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5).to(DT[ft]).to(dev)  # noqa: E731
    gbar, pbar = [rnd((n_col, n_lev)) for _ in range(4)], [rnd((n_col,)) for _ in range(2)]
    ot, op = torch.empty((4, n_col, n_lev), dtype=DT[ft], device=dev), torch.empty((2, n_col), dtype=DT[ft], device=dev)
    tab = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    in_p, out_p = tab(cols), tab(list(ot))
    keep = [structs, cols, gbar, pbar, ot, op, inv_dz, in_p, out_p]

    # the primal entry through a plain ctypes handle: --primal-only must also load a library that has no §28 symbols
    fn = getattr(C.CDLL(str(_lib.LIB_PATH)), f"cmx_mp1m_column_tendencies_sedimentation_{ft}")
    fn.restype = C.c_int32
    real = C.c_float if ft == "f32" else C.c_double
    fn.argtypes = [C.c_void_p] * 5 + [C.c_uint32, real, real, C.c_int32, C.c_int64, C.c_int32] + [C.c_void_p] * 6
    pargs = (C.addressof(mp.c), C.addressof(tps), C.addressof(stokes), C.addressof(cr), C.addressof(ci), mp.flags, 0.0, 0.0, 0, n_col, n_lev,
             inv_dz.data_ptr(), C.addressof(in_p), C.addressof(out_p), op[0].data_ptr(), op[1].data_ptr())

    def primal():
        assert fn(*pargs, torch.cuda.current_stream(dev).cuda_stream) == 0
    cases = {f"{ft} primal column step": primal}
    if primal_only:
        return cases, keep
    ndir = len(NAMES)
    quints = [P.column_parameter_direction_1m(mp, {k: P.DEFAULT_PARAMETERS[P.split_indexed_name(k)[0]][P.split_indexed_name(k)[1]]
                                                   if P.split_indexed_name(k)[1] is not None else P.DEFAULT_PARAMETERS[k]}) for k in NAMES]
    tables = [(type(quints[0][k]) * ndir)(*[q[k] for q in quints]) for k in range(5)]
    dirs = [C.byref(t[0]) for t in tables]
    oj, ojp = torch.empty((KP[ft], 4, n_col, n_lev), dtype=DT[ft], device=dev), torch.empty((2, ndir, n_col), dtype=DT[ft], device=dev)
    grad = torch.empty(ndir, dtype=torch.float64, device=dev)
    ws = torch.empty(ndir * _abi.CMX_PARAM_VJP_PARTIALS, dtype=torch.float64, device=dev)
    head = (C.byref(mp.c), C.byref(tps), C.byref(stokes), C.byref(cr), C.byref(ci), mp.flags, n_col, n_lev, ptr(inv_dz), in_p)
    keep += [tables, oj, ojp, grad, ws]
    # the 16-direction J_θ δθ writes every direction's four columns over the SAME KP blocks of output (16 × 4 columns of 1e7 points would not be what a caller
    # keeps either: a calibration contracts them); the precipitation columns are all kept
    jv16 = tab([oj[d % KP[ft], o] for d in range(ndir) for o in range(4)])

    def central():
        for _ in range(2 * ndir):
            primal()

    def jvp_kp():
        _lib.call("cmx_mp1m_column_param_jvp", fam, dev, *head, KP[ft], *dirs, tab([oj[d, o] for d in range(KP[ft]) for o in range(4)]),
                  tab(list(ojp[0, :KP[ft]])), tab(list(ojp[1, :KP[ft]])), None, None, None)

    def jvp_16():
        _lib.call("cmx_mp1m_column_param_jvp", fam, dev, *head, ndir, *dirs, jv16, tab(list(ojp[0])), tab(list(ojp[1])), None, None, None)

    def grad_16():
        _lib.call("cmx_mp1m_column_param_vjp", fam, dev, *head, tab(gbar), ptr(pbar[0]), ptr(pbar[1]), ndir, *dirs, ptr(grad), ptr(ws), None, None, None)
    cases.update({f"{ft} {2 * ndir} primal calls (central differences, 16 names)": central, f"{ft} J_θ δθ, {KP[ft]} directions (one launch)": jvp_kp,
                  f"{ft} J_θ δθ, 16 directions": jvp_16, f"{ft} gradient, 16 names": grad_16})
    return cases, keep


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--levels", type=int, default=64)
    ap.add_argument("--primal-only", action="store_true")
    ap.add_argument("sizes", nargs="*", type=lambda a: int(float(a)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {cmx._lib.LIB_PATH}")
    for n in args.sizes or [10_000_000]:
        n_col = n // args.levels
        cases, keep = {}, []
        for ft in ("f32", "f64"):
            c, k = cases_of(ft, n_col, args.levels, dev, args.primal_only)
            cases.update(c)
            keep.append(k)
        for fn in cases.values():                   # warm-up
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in cases}
        for _ in range(args.runs):
            times = {k: [] for k in cases}
            for _ in range(TJ.ROUNDS):              # alternating: every case once per round
                for k, fn in cases.items():
                    times[k].append(TJ.timed(fn))
            for k, t in times.items():
                runs[k].append(statistics.median(t))
        print(f"{'case':<60} {'points':>10} {'levels':>6} {'ms (median of the runs)':>24} {'runs, ms':>30} {'vs primal':>9}")
        for k, r in runs.items():
            base = statistics.median(runs[f"{k[:3]} primal column step"])
            print(f"{k:<60} {n_col * args.levels:>10d} {args.levels:>6d} {statistics.median(r):>24.3f} {' '.join(f'{t:.3f}' for t in r):>30} {statistics.median(r) / base:>9.2f}",
                  flush=True)


if __name__ == "__main__":
    main()
