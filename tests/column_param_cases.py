"""What tests/test_column_param_host.py and tests/test_column_param_gpu.py share: the derivatives of the SB2006 COLUMN step — tendencies, fall speeds, upwind
flux divergence and the surface precipitation flux — with respect to the scheme's PARAMETERS (include/cmx.h §26).

REFERENCE.  Central differences of the Float64 ORACLE's column step (oracle_binding.sb2006_column_tendencies_sedimentation) with respect to one ClimaParams name
at a time: θ_p ± h with h = 1e-6·|θ_p| (and 4h), ALL FOUR parameter structs rebuilt by the constructors of cmx.parameters from the overridden dictionary, the
quotient formed with the realised θ⁺ − θ⁻, held as logarithmic sensitivities S = ∂out/∂θ_p·θ_p.  The code under test returns S directly: its direction for
name p is `column_parameter_direction(params, {p: θ_p})`.

MEASURE: that of tests/param_cases.py (row_error: e = |S − S^ref| / s_o, s_o the row scale over the tested names; AGREE, BOUND, LOW_SHARE, dead parameters), with
the precipitation flux as a FIFTH row with its own scale, one value per column.  A point is kept if the references at h and 4h agree within AGREE in all four
tendency rows, a column's precipitation row likewise; at most MAX_SET_ASIDE (1 %) of the points and of the columns may be set aside (asserted where the
reference is built).

NAMES: those of tests/param_cases.py plus the rain fall-speed coefficients aR, bR, cR and the gravitational acceleration.
STATES and SHAPES: the columns of tests/column_products_cases.py (interior states, the rain removed at every 13th point).  The new kernel has that file's
tiling — one point per lane, a workgroup owns 255 points — so n7 (120 × 7: tile boundaries inside columns at levels 3, 6 and 2), n1 (64 × 1), n2 (32 × 2) and
n3 (2 × 3) are the shapes here too."""
import ctypes as C
import functools

import numpy as np

import column_products_cases as CC
import param_cases as PC
from jacobian_host_build import CT, NPT, _arr, _same_bits, host_fixture  # noqa: F401
from cmx import _abi
from cmx import parameters as P

host = host_fixture("column_param_host")
BOUND, AGREE, MAX_SET_ASIDE, LOW_SHARE = PC.BOUND, PC.AGREE, PC.MAX_SET_ASIDE, PC.LOW_SHARE
NEW_NAMES = ("SB2006_raindrops_terminal_velocity_coeff_aR", "SB2006_raindrops_terminal_velocity_coeff_bR", "SB2006_raindrops_terminal_velocity_coeff_cR",
             "gravitational_acceleration")
NAMES = PC.NAMES + NEW_NAMES
EXPONENTS = PC.EXPONENTS
CASES, CASE_IDS, MAIN_CASE, SHAPES, VEL_KIND = CC.CASES, CC.CASE_IDS, CC.MAIN_CASE, CC.SHAPES, CC.VEL_KIND
OUT = PC.OUT


def theta(names=NAMES):
    return np.array([P.DEFAULT_PARAMETERS[k] for k in names], dtype=np.float64)


def params(ft, case, ov=None):
    """(warm-rain parameters, thermodynamics, rain fall speed, Stokes cloud fall speed or None), all four from ONE overridden dictionary."""
    td = P.create_toml_dict(ft, ov or {})
    vel = P.rain_vel_params(td)
    if case[1] == "chen_gen":
        vel.chen2022.b_rho = 0.6          # a table that make_chen_log rejects: the general Chen-2022 instantiation (run-time Γ)
    return P.WarmRainParams2M(td, case[0]), P.ThermodynamicsParameters(td), vel, P.StokesRegimeVelType(td) if case[2] else None


def directions(ft, case, names=NAMES):
    """(wr, tps, vel, stokes, [d_wr, d_tps, d_vel, d_stokes] tables of len(names)): direction p is θ_p along name p, so a jvp column is S_·p."""
    wr, tps, vel, stokes = params(ft, case)
    quads = [P.column_parameter_direction(wr, {k: float(t)}, vel, stokes) for k, t in zip(names, theta(names))]
    tables = [(type(quads[0][k]) * len(quads))(*[q[k] for q in quads]) for k in range(4)]
    return wr, tps, vel, stokes, tables


# ---- the reference --------------------------------------------------------------------------------------------------------------------------------
def oracle_column(case, ov, inv_dz, cols):
    import oracle_binding as oracle
    wr, tps, vel, stokes = params("f64", case, ov)
    r = oracle.sb2006_column_tendencies_sedimentation(_abi.F64, wr.c, tps, vel, stokes, CC.flags(case), inv_dz, *cols, float32_gates=False, nthreads=4)
    return np.stack([r[k] for k in OUT]), np.array(r["precip_flux"])


def fd_sensitivities(case, inv_dz, cols, names, step):
    """(S [4, P, n], S_precip [1, P, n_col]) by central differences of the oracle with h = step·|θ_p|."""
    n_col, n_lev = cols[0].shape
    S, Sp = np.empty((4, len(names), n_col * n_lev)), np.empty((1, len(names), n_col))
    for p, (k, t) in enumerate(zip(names, theta(names))):
        h = step * abs(t)
        tp, tm = t + h, t - h
        (yp, pp), (ym, pm) = oracle_column(case, {k: tp}, inv_dz, cols), oracle_column(case, {k: tm}, inv_dz, cols)
        S[:, p] = (yp - ym) / (tp - tm) * t
        Sp[0, p] = (pp - pm) / (tp - tm) * t
    return S, Sp


@functools.lru_cache(maxsize=None)
def _reference(case, shape):
    import oracle_binding as oracle
    oracle.lib()
    inv_dz, cols = CC.columns(shape)
    (S1, P1), (S4, P4) = fd_sensitivities(case, inv_dz, cols, NAMES, 1e-6), fd_sensitivities(case, inv_dz, cols, NAMES, 4e-6)
    dis, disp = PC.row_error(S1, S4).max(axis=(0, 1)), PC.row_error(P1, P4).max(axis=(0, 1))
    kept, keptp = dis <= AGREE, disp <= AGREE
    dead = np.array([not S1[:, p].any() and not S4[:, p].any() for p in range(len(NAMES))])
    deadp = np.array([not P1[:, p].any() and not P4[:, p].any() for p in range(len(NAMES))])
    ref = dict(case=case, shape=shape, n_col=cols[0].shape[0], n_lev=cols[0].shape[1], inv_dz=inv_dz, cols=cols, S=S1, Sp=P1, S4=S4, Sp4=P4, kept=kept, keptp=keptp, dead=dead,
               deadp=deadp, worst=float(max(dis[kept].max(initial=0.0), disp[keptp].max(initial=0.0))))
    for a in (S1, P1, S4, P4, kept, keptp, dead, deadp):
        a.setflags(write=False)
    return ref


def reference_unchecked(case, shape):
    return _reference(tuple(case), shape)


def set_aside_shares(ref):
    return float((~ref["kept"]).mean()), float((~ref["keptp"]).mean())


def reference(case, shape):
    """The reference of (case, shape), computed once and shared read-only; asserts the 1 % condition where it is built."""
    ref = reference_unchecked(case, shape)
    pts, cls = set_aside_shares(ref)
    assert pts <= MAX_SET_ASIDE and cls <= MAX_SET_ASIDE, (case, shape, pts, cls)
    return ref


# ---- the measure ----------------------------------------------------------------------------------------------------------------------------------
def _shares(S_ref, kept):
    A = np.abs(S_ref)[:, :, kept]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.nan_to_num(A / A.max(axis=1, keepdims=True)).max(axis=(0, 2))


def worst_errors(ref, S, Sp):
    """([P] worst row error of the tendencies over the kept points, [P] of the precipitation row over the kept columns)."""
    return PC.row_error(S, ref["S"])[:, :, ref["kept"]].max(axis=(0, 2)), PC.row_error(Sp, ref["Sp"])[:, :, ref["keptp"]].max(axis=(0, 2))


def assert_parity(ft, ref, S, Sp, what, report=True):
    """Every (row, parameter) of every kept point / column inside BOUND[ft]; every dead parameter exactly zero EVERYWHERE; Float64: the low-share columns also
    in their own scale.  S: [P, 4, n] (the jvp layout), Sp: [P, n_col]."""
    S = np.asarray(S, dtype=np.float64).transpose(1, 0, 2)
    Sp = np.asarray(Sp, dtype=np.float64)[None]
    e, ep = worst_errors(ref, S, Sp)
    if report:
        print(f"{what} {ft} {ref['case']} {ref['shape']}: kept {int(ref['kept'].sum())}/{ref['kept'].size} points, {int(ref['keptp'].sum())}/{ref['keptp'].size} "
              f"columns, h-vs-4h {ref['worst']:.3g}; worst error — tendencies {e.max():.3g} ({NAMES[int(e.argmax())]}), precipitation {ep.max():.3g} "
              f"({NAMES[int(ep.argmax())]}); dead in the precipitation row: {int(ref['deadp'].sum())}")
    for p in np.nonzero(ref["dead"])[0]:
        assert not S[:, p].any(), (what, NAMES[p], "dead in the reference, not exactly zero")
    for p in np.nonzero(ref["deadp"])[0]:
        assert not Sp[:, p].any(), (what, NAMES[p], "dead in the reference's precipitation row, not exactly zero")
    for p in np.nonzero(~(e < BOUND[ft]))[0]:
        raise AssertionError((what, "tendencies", NAMES[p], float(e[p])))
    for p in np.nonzero(~(ep < BOUND[ft]))[0]:
        raise AssertionError((what, "precipitation", NAMES[p], float(ep[p])))
    if ft == "f64":
        # LOW_SHARE (tests/param_cases.py): a live parameter whose largest row share stays below 0.02 is also held in the column's own scale, 1e-5·max_i |S^ref|
        # per row — on the rows whose column the reference itself resolves: its values at h and 4h agree there to 1e-6 of that scale, ten times inside the bound
        # (on the small shapes a column of a few dozen points can lie below the rounding of the difference quotient, 1e-10 of the row's size; printed then)
        for rows, Sx, Sr, S4, kept, dead in ((4, S, ref["S"], ref["S4"], ref["kept"], ref["dead"]), (1, Sp, ref["Sp"], ref["Sp4"], ref["keptp"], ref["deadp"])):
            sh = _shares(Sr, kept)
            for p in [p for p in range(len(NAMES)) if not dead[p] and sh[p] < LOW_SHARE]:
                d = np.abs(Sx[:, p][:, kept] - Sr[:, p][:, kept]).max(axis=1)
                scale = np.abs(Sr[:, p][:, kept]).max(axis=1)
                resolved = np.abs(S4[:, p][:, kept] - Sr[:, p][:, kept]).max(axis=1) <= 1e-6 * scale
                if report:
                    print(f"  {what}: low share {sh[p]:.2g} {NAMES[p]} ({rows} rows): column-scale error {np.max(d / np.where(scale > 0, scale, 1.0)):.3g}, "
                          f"rows the reference resolves: {resolved.tolist()}")
                assert (d <= 1e-5 * scale)[resolved].all(), (what, NAMES[p], d, scale)
    return e, ep


def grad_from_jvp(g, pbar, jv, jp):
    """[P] Σ ḡ·jvp + Σ p̄·ṗ in float64, and [P] Σ |ḡ·jvp| + Σ |p̄·ṗ|: what the gradient entry's sum is compared with and the size of its terms."""
    g, jv = np.asarray(g, dtype=np.float64), np.asarray(jv, dtype=np.float64)
    t = (g[None] * jv).reshape(jv.shape[0], -1)
    tp = np.asarray(pbar, dtype=np.float64)[None] * np.asarray(jp, dtype=np.float64)
    return t.sum(axis=1) + tp.sum(axis=1), np.abs(t).sum(axis=1) + np.abs(tp).sum(axis=1)


def cotangents(ref, seed=7):
    """(ḡ [4, n], p̄ [n_col]): every output weighed alike, ḡ_o = r / (largest |S^ref| of the row at the point), as tests/column_products_cases.py does."""
    rng = np.random.default_rng(seed)
    s, sp = np.abs(ref["S"]).max(axis=1), np.abs(ref["Sp"]).max(axis=1)[0]
    r = rng.uniform(0.5, 1.0, s.shape) * rng.choice([-1.0, 1.0], s.shape)
    rp = rng.uniform(0.5, 1.0, sp.shape) * rng.choice([-1.0, 1.0], sp.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, r / s, 0.0), np.where(sp > 0, rp / sp, 0.0)


# ---- calls into the host build --------------------------------------------------------------------------------------------------------------------
def _flat(ft, a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=NPT[ft]) if a is not None else None


def _ptr(ft, a):
    return a.ctypes.data_as(C.POINTER(CT[ft])) if a is not None else None


def _head(structs, case, override_flags=None):
    wr, tps, vel, stokes = structs
    return (C.byref(wr.c), C.byref(tps), C.byref(vel), C.byref(stokes) if stokes is not None else None,
            C.c_uint32(CC.flags(case) if override_flags is None else override_flags))


def _dirs(tables, lo=0, use=(True, True, True, True)):
    return [C.byref(t[lo]) if t is not None and u else None for t, u in zip(tables, use)]


def host_jvp(host, ft, case, structs, inv_dz, cols, tables, lo=0, ndir=None, kp=0, with_primal=True, override_flags=None, use=(True,) * 4, sentinel=-7.0):
    """(jvp [ndir, 4, n], jvp_precip [ndir, n_col], tendencies [4, n], precip [n_col], status ≥ 0: the velocity kind that ran) of the host build, for the
    directions lo … lo + ndir − 1 of the tables."""
    n_col, n_lev = np.shape(cols[0])
    n = n_col * n_lev
    ndir = len(tables[0]) - lo if ndir is None else ndir
    if _abi.CMX_PARAM_MAX_DIRS < ndir <= len(tables[0]) - lo:      # several calls of the entry, as the wrappers make them; the primal outputs are the first call's
        parts = [host_jvp(host, ft, case, structs, inv_dz, cols, tables, lo + d0, min(_abi.CMX_PARAM_MAX_DIRS, ndir - d0), kp, with_primal and d0 == 0,
                          override_flags, use, sentinel) for d0 in range(0, ndir, _abi.CMX_PARAM_MAX_DIRS)]
        return np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts]), parts[0][2], parts[0][3], min(q[4] for q in parts)
    x, dz = [_flat(ft, c) for c in cols], _flat(ft, inv_dz)
    jv, jp = np.full((max(ndir, 1), 4, n), sentinel, dtype=NPT[ft]), np.full((max(ndir, 1), n_col), sentinel, dtype=NPT[ft])
    tend, pr = np.full((4, n), sentinel, dtype=NPT[ft]), np.full(n_col, sentinel, dtype=NPT[ft])
    fn = getattr(host, f"host_sb2006_column_param_jvp_{ft}")
    fn.restype = C.c_int32
    rc = fn(*_head(structs, case, override_flags), C.c_int(kp), C.c_int64(n_col), C.c_int32(n_lev), _ptr(ft, dz), _arr(ft, x), C.c_int32(ndir), *_dirs(tables, lo, use),
            _arr(ft, [jv[d, o] for d in range(jv.shape[0]) for o in range(4)]), _arr(ft, list(jp)), _arr(ft, list(tend)) if with_primal else None,
            _ptr(ft, pr) if with_primal else None)
    return jv, jp, tend, pr, rc


def host_vjp(host, ft, case, structs, inv_dz, cols, g, pbar, tables, lo=0, ndir=None, kp=0, with_primal=False, override_flags=None, use=(True,) * 4, sentinel=-7.0):
    """(grad [ndir] float64, tendencies [4, n], precip [n_col], status) of the host build."""
    n_col, n_lev = np.shape(cols[0])
    n = n_col * n_lev
    ndir = len(tables[0]) - lo if ndir is None else ndir
    if _abi.CMX_PARAM_MAX_DIRS < ndir <= len(tables[0]) - lo:
        parts = [host_vjp(host, ft, case, structs, inv_dz, cols, g, pbar, tables, lo + d0, min(_abi.CMX_PARAM_MAX_DIRS, ndir - d0), kp, with_primal and d0 == 0,
                          override_flags, use, sentinel) for d0 in range(0, ndir, _abi.CMX_PARAM_MAX_DIRS)]
        return np.concatenate([q[0] for q in parts]), parts[0][1], parts[0][2], min(q[3] for q in parts)
    x, dz = [_flat(ft, c) for c in cols], _flat(ft, inv_dz)
    cot = [_flat(ft, a) for a in g] if g is not None else None
    pb = _flat(ft, pbar)
    grad = np.full(max(ndir, 1), sentinel, dtype=np.float64)
    tend, pr = np.full((4, n), sentinel, dtype=NPT[ft]), np.full(n_col, sentinel, dtype=NPT[ft])
    fn = getattr(host, f"host_sb2006_column_param_vjp_{ft}")
    fn.restype = C.c_int32
    rc = fn(*_head(structs, case, override_flags), C.c_int(kp), C.c_int64(n_col), C.c_int32(n_lev), _ptr(ft, dz), _arr(ft, x), _arr(ft, cot) if cot is not None else None,
            _ptr(ft, pb), C.c_int32(ndir), *_dirs(tables, lo, use), grad.ctypes.data_as(C.POINTER(C.c_double)), _arr(ft, list(tend)) if with_primal else None,
            _ptr(ft, pr) if with_primal else None)
    return grad, tend, pr, rc
