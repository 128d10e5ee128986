"""HIP-event times of the parameter-ensemble entries (include/cmx.h §29) beside what they replace: ONE ensemble call against E calls of the single entry of
the SAME library in the same process, for the four families and both float types.  The host-side folds of the single calls are inside the timed region —
that is what a caller pays per member and step; the ensemble table is packed and copied once, outside (it is reused across steps).  Every output is
allocated once; the entries are called through the raw ABI.  All cases alternate in one session (every case once per round, median of 7 rounds of 5
calls); the session is repeated `--runs` times.
    (a) E = 128 members of one 64-level column (pointwise: 64 points) — the single-column calibration
    (b) E = 32 members of 1e5 points, every member its own state
    (c) the same with CMX_ENSEMBLE_SHARED_STATE
With `--single-only` only the four single entries are timed, at `--points` (default 1e7), through a plain handle of the library CMX_LIB names: run so with
the library of another build, in alternating processes, to see that the single entries did not move.
With `--implicit` the two implicit column steps of §(21) are timed instead (Δt = 300 s, nsub = 2, nonnegative), in the same three cases or `--single-only`.
    python tools/time_ensemble.py [--runs 3] [--single-only] [--points 1e7] [--implicit]"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "cloudmicrophysics.jl_amd"))
import time_jacobian as TJ  # noqa: E402
import cmx  # noqa: E402
from cmx import _abi, _lib  # noqa: E402
from cmx import parameters as P  # noqa: E402

DT = TJ.DT
LEVELS = 64
FAMILIES = ("SB2006 tendencies", "1-moment tendencies", "SB2006 column step", "1-moment column step", "SB2006 implicit column step",
            "1-moment implicit column step")
EXPLICIT, IMPLICIT = FAMILIES[:4], FAMILIES[4:]
STEP = (300.0, 2, _abi.CMX_STEP_NONNEGATIVE)      # Δt, nsub, step flags of the implicit column steps


def _members(ft, fam, E):
    """E parameter sets, each with one rate coefficient moved by up to ±10 % (the instantiation stays the default one)."""
    out = []
    for e in range(E):
        f = 1.0 + 0.2 * (e / max(E - 1, 1) - 0.5)
        if fam.startswith("SB2006"):
            m = P.WarmRainParams2M(ft)
            m.c.seifert_beheng.acnv.kcc *= f
        else:
            m = P.Microphysics1MParams(ft)
            m.c.process_params.e_lcl_rai *= f
        out.append(m)
    return out


def _single_fn(lib, fam, ft):
    """(function with argtypes of plain pointers, so that a library without the §29 symbols can be timed too)"""
    real = C.c_float if ft == "f32" else C.c_double
    vp, u32, i32, i64 = C.c_void_p, C.c_uint32, C.c_int32, C.c_int64
    name, argtypes = {
        FAMILIES[0]: ("cmx_sb2006_warm_rain_tendencies", [vp, vp, vp, u32, i64] + [vp] * 14),
        FAMILIES[1]: ("cmx_mp1m_tendencies", [vp, vp, u32, i64] + [vp] * 12),
        FAMILIES[2]: ("cmx_sb2006_column_tendencies_sedimentation", [vp, vp, vp, vp, u32, i64, i32] + [vp] * 14),
        FAMILIES[3]: ("cmx_mp1m_column_tendencies_sedimentation", [vp] * 5 + [u32, real, real, i32, i64, i32] + [vp] * 6),
        FAMILIES[4]: ("cmx_sb2006_column_implicit_step", [vp, vp, vp, vp, u32, C.c_double, i32, u32, i64, i32] + [vp] * 14),
        FAMILIES[5]: ("cmx_mp1m_column_implicit_step", [vp] * 5 + [u32, C.c_double, i32, u32, i64, i32] + [vp] * 6),
    }[fam]
    fn = getattr(lib, f"{name}_{ft}")
    fn.restype, fn.argtypes = i32, argtypes
    return fn


def cases_of(ft, fam, E, n_col, shared, dev, lib, single_only=False):
    """{label: callable} for one family: E single calls, and (unless single_only) one ensemble call."""
    col = "column" in fam
    n = n_col * LEVELS if col else n_col
    states = TJ.states_sb2006 if fam.startswith("SB2006") else TJ.states_mp1m
    lead = 1 if shared else E
    cols = [c.to(DT[ft]).to(dev).reshape(lead, n).contiguous() for c in states(lead * n)]
    out = [torch.empty((E, n), dtype=DT[ft], device=dev) for _ in range(4)]
    precip = [torch.empty((E, n_col), dtype=DT[ft], device=dev) for _ in range(2)]
    inv_dz = (1.0 / torch.linspace(40.0, 400.0, LEVELS, dtype=torch.float64)).to(DT[ft]).to(dev)
    mps, tps = _members(ft, fam, E), P.ThermodynamicsParameters(ft)
    vel, stokes, cr, ci = P.rain_vel_params(ft), P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft), P.Chen2022VelTypeIce(ft)
    adr, ptr = C.addressof, lambda t: t.data_ptr()      # noqa: E731
    fn = _single_fn(lib, fam, ft)
    keep = [cols, out, precip, inv_dz, mps, tps, vel, stokes, cr, ci]
    flags2 = _abi.CMX_SB2006_LIMITED | _abi.CMX_VEL_SB2006
    tabs = []
    if fam in (FAMILIES[3], FAMILIES[5]):
        tabs = [((C.c_void_p * 7)(*[ptr(c[0 if shared else e]) for c in cols]), (C.c_void_p * 4)(*[ptr(o[e]) for o in out])) for e in range(E)]
        keep.append(tabs)

    def single(e, s):
        x = [ptr(c[0 if shared else e]) for c in cols]
        y = [ptr(o[e]) for o in out]
        if fam == FAMILIES[0]:
            return fn(adr(mps[e].c), adr(tps), None, _abi.CMX_SB2006_LIMITED, n, *x, *y, None, None, s)
        if fam == FAMILIES[1]:
            return fn(adr(mps[e].c), adr(tps), mps[e].flags, n, *x, *y, s)
        if fam == FAMILIES[2]:
            return fn(adr(mps[e].c), adr(tps), adr(vel), None, flags2, n_col, LEVELS, ptr(inv_dz), *x, *y, ptr(precip[0][e]), s)
        if fam == FAMILIES[4]:
            return fn(adr(mps[e].c), adr(tps), adr(vel), None, flags2, *STEP, n_col, LEVELS, ptr(inv_dz), *x, *y, ptr(precip[0][e]), s)
        if fam == FAMILIES[5]:
            return fn(adr(mps[e].c), adr(tps), adr(stokes), adr(cr), adr(ci), mps[e].flags, *STEP, n_col, LEVELS, ptr(inv_dz), adr(tabs[e][0]),
                      adr(tabs[e][1]), ptr(precip[0][e]), ptr(precip[1][e]), s)
        return fn(adr(mps[e].c), adr(tps), adr(stokes), adr(cr), adr(ci), mps[e].flags, 0.0, 0.0, 0, n_col, LEVELS, ptr(inv_dz), adr(tabs[e][0]),
                  adr(tabs[e][1]), ptr(precip[0][e]), ptr(precip[1][e]), s)

    def singles():
        s = torch.cuda.current_stream(dev).cuda_stream
        for e in range(E):
            assert single(e, s) == 0

    layout = "shared state" if shared else "member-major"
    label = f"{ft} {fam}, E = {E} x {n} points, {layout}"
    cases = {f"{label}: {E} single calls": singles}
    if single_only:
        return cases, keep
    from cmx import ensemble as ens
    if fam.startswith("SB2006"):
        table = ens.pack_2m(mps, tps, vel=cmx.SB2006VelType if col else None).to(dev)
    else:
        table = ens.pack_1m(mps, tps, **(dict(stokes=stokes, chen_rain=cr, chen_ice=ci) if col else {})).to(dev)
    keep.append(table)
    fam_abi = _abi.F32 if ft == "f32" else _abi.F64
    head = (C.byref(table.desc), C.c_void_p(table.table.data_ptr()), E, _abi.CMX_ENSEMBLE_SHARED_STATE if shared else 0)
    x, y = [C.c_void_p(ptr(c)) for c in cols], [C.c_void_p(ptr(o)) for o in out]
    in_p, out_p = (C.c_void_p * 7)(*[ptr(c) for c in cols]), (C.c_void_p * 4)(*[ptr(o) for o in out])
    keep += [in_p, out_p]

    def ensemble():
        if fam == FAMILIES[0]:
            _lib.call("cmx_sb2006_warm_rain_tendencies_ensemble", fam_abi, dev, *head, n, *x, *y, None, None)
        elif fam == FAMILIES[1]:
            _lib.call("cmx_mp1m_tendencies_ensemble", fam_abi, dev, *head, n, *x, *y)
        elif fam == FAMILIES[2]:
            _lib.call("cmx_sb2006_column_tendencies_sedimentation_ensemble", fam_abi, dev, *head, n_col, LEVELS, C.c_void_p(ptr(inv_dz)), *x, *y,
                      C.c_void_p(ptr(precip[0])))
        elif fam == FAMILIES[4]:
            _lib.call("cmx_sb2006_column_implicit_step_ensemble", fam_abi, dev, *head, *STEP, n_col, LEVELS, C.c_void_p(ptr(inv_dz)), *x, *y,
                      C.c_void_p(ptr(precip[0])))
        elif fam == FAMILIES[5]:
            _lib.call("cmx_mp1m_column_implicit_step_ensemble", fam_abi, dev, *head, *STEP, n_col, LEVELS, C.c_void_p(ptr(inv_dz)), in_p, out_p,
                      C.c_void_p(ptr(precip[0])), C.c_void_p(ptr(precip[1])))
        else:
            _lib.call("cmx_mp1m_column_tendencies_sedimentation_ensemble", fam_abi, dev, *head, 0.0, 0.0, 0, n_col, LEVELS, C.c_void_p(ptr(inv_dz)), in_p,
                      out_p, C.c_void_p(ptr(precip[0])), C.c_void_p(ptr(precip[1])))
    cases[f"{label}: one ensemble call"] = ensemble
    return cases, keep


def session(cases, runs):
    for fn in cases.values():                   # warm-up
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in cases}
    for _ in range(runs):
        times = {k: [] for k in cases}
        for _ in range(TJ.ROUNDS):              # alternating: every case once per round
            for k, fn in cases.items():
                times[k].append(TJ.timed(fn))
        for k, t in times.items():
            res[k].append(statistics.median(t))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--points", type=lambda a: int(float(a)), default=10_000_000)
    ap.add_argument("--implicit", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {_lib.LIB_PATH}")
    lib = C.CDLL(str(_lib.LIB_PATH))
    cases, keep = {}, []
    families = IMPLICIT if args.implicit else EXPLICIT
    if args.single_only:
        for ft in ("f32", "f64"):
            for fam in families:
                c, k = cases_of(ft, fam, 1, args.points // LEVELS if "column" in fam else args.points, False, dev, lib, single_only=True)
                cases.update(c)
                keep.append(k)
    else:
        for ft in ("f32", "f64"):
            for fam in families:
                col = "column" in fam
                for E, n_col, shared in ((128, 1 if col else LEVELS, False), (32, 100_000 // LEVELS if col else 100_000, False),
                                         (32, 100_000 // LEVELS if col else 100_000, True)):
                    c, k = cases_of(ft, fam, E, n_col, shared, dev, lib)
                    cases.update(c)
                    keep.append(k)
    res = session(cases, args.runs)
    print(f"{'case':<100} {'ms (median of the runs)':>24} {'runs, ms':>30} {'E singles / ensemble':>21}")
    for k, r in res.items():
        ratio = ""
        if k.endswith("one ensemble call"):
            base = k.rsplit(": ", 1)[0]
            single = [s for s in res if s.startswith(base + ": ") and s.endswith("single calls")][0]
            ratio = f"{statistics.median(res[single]) / statistics.median(r):.2f}"
        print(f"{k:<100} {statistics.median(r):>24.4f} {' '.join(f'{t:.4f}' for t in r):>30} {ratio:>21}", flush=True)


if __name__ == "__main__":
    main()
