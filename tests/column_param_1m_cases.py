"""What tests/test_column_param_1m_host.py and tests/test_column_param_1m_gpu.py share: the derivatives of the 1-moment COLUMN step — tendencies, the four fall
speeds, the upwind flux divergence and the surface fluxes of rain and snow — with respect to the scheme's PARAMETERS (include/cmx.h §28).

REFERENCE.  Central differences of the Float64 ORACLE's column step (oracle_binding.mp1m_column_tendencies_sedimentation, nsub = 0, float32_gates=False) with
respect to one name at a time: θ_p ± h with h = 1e-6·|θ_p| (and 4h), ALL FIVE parameter structs rebuilt by the constructors of cmx.parameters from the ONE
overridden dictionary (an entry of a vector-valued name, "Chen2022_table_B5_Al[1]", overrides that entry of the list), the quotient formed with the realised
θ⁺ − θ⁻, held as logarithmic sensitivities S = ∂out/∂θ_p·θ_p.  The code under test returns S directly: its direction for name p is
`column_parameter_direction_1m(mp, {p: θ_p})`.

NAMES: `parameters.COLUMN_1M_DIRECTION_NAMES` with θ_p ≠ 0 in the case's dictionary.

MEASURE: that of tests/param_cases.py unchanged (row_error: e = |S − S^ref| / s_o, s_o the row scale over the tested names; AGREE, BOUND, LOW_SHARE, the exact zero
of dead parameters), with the two precipitation fluxes as a FIFTH and a SIXTH row, each with its own scale, one value per column.  A point is kept if the
references at h and 4h agree within AGREE in all four tendency rows, a column's precipitation rows likewise; at most MAX_SET_ASIDE (1 %) of the points and of
the columns may be set aside (asserted where the reference is built).

TWO NAMES THAT LOOK DEAD BUT ARE NOT: Chen2022_table_B5_Fl[2] and Chen2022_table_B5_Hl[2] enter the large-ice fold as exp(log(−θ) − ρᵢ) with ρᵢ of snow: about
1e-24 of the constant they are added to, below the rounding of the difference quotient, so the reference comes out identically zero.  The analytic tangent is
tiny and NOT zero; these two are held to the row bound only, not to exact zero (NOT_STRUCTURALLY_DEAD).

DEAD NAMES ON THE SMALL SHAPES.  Whether a name is dead — reaches no output, so that the code under test must return exact zeros — is a property of the name,
the case and the set, not of how many columns are looked at; it is decided on the 840 points of n7 and used for n1, n2 and n3 of the same case and set.  On
a handful of columns a LIVE name can difference to exact zeros by coincidence of rounding: rain_drop_length_scale cancels analytically in the slope
parameter (m0 ∝ r0^me against r0^(me + Δm), Δm = 0) and survives only as the rounding residue of that cancellation, 1e-16 of the row, which the oracle's
quotient reproduces as exact zeros in both columns of n3 and as noise of that size on n7.  Such a name is held to the row bound there, as everywhere.

STATES, CASES and SHAPES: tests/column_products_1m_cases.py — the sets cold and warm; default, alt, exponents, and default with the general-Γ rain table
(b_ρ = 0.6); n7 (120 × 7: tile boundaries inside columns at levels 3, 6 and 2), n1 (64 × 1), n2 (32 × 2), n3 (2 × 3)."""
import ctypes as C
import functools

import numpy as np

import column_products_1m_cases as K1
import param_1m_cases as P1
import param_cases as PC
from jacobian_host_build import CT, NPT, _arr, _same_bits, host_fixture  # noqa: F401
from cmx import _abi
from cmx import parameters as P

host = host_fixture("column_param_1m_host")
BOUND, AGREE, MAX_SET_ASIDE, LOW_SHARE = PC.BOUND, PC.AGREE, PC.MAX_SET_ASIDE, PC.LOW_SHARE
CASES, CASE_IDS, MAIN_CASE, SHAPES, WHICH, KIND = K1.CASES, K1.CASE_IDS, K1.MAIN_CASE, K1.SHAPES, K1.WHICH, K1.KIND
OUT, PRECIP = K1.OUT, K1.PRECIP
NOT_STRUCTURALLY_DEAD = ("Chen2022_table_B5_Fl[2]", "Chen2022_table_B5_Hl[2]")
EXPONENT_NAMES = P1.EXPONENT_NAMES
# names that reach the outputs through sedimentation only
SEDIMENTATION_ONLY = ("cloud_liquid_sedimentation_number_concentration", "cloud_ice_sedimentation_number_concentration", "snow_aspect_ratio",
                      "snow_aspect_ratio_coefficient", "Chen2022_table_B1_q_coeff", "Chen2022_table_B1_ai[0]", "Chen2022_table_B3_As[0]", "Chen2022_table_B5_Al[0]",
                      "Chen2022_table_B5_Cl[1]", "Chen2022_table_B5_El[0]")


# ---- names and parameters ---------------------------------------------------------------------------------------------------------------------------
def _value(d, name):
    base, idx = P.split_indexed_name(name)
    v = d.get(base, P.DEFAULT_PARAMETERS[base])
    return float(v if idx is None else v[idx])


def overrides(case):
    return P1.overrides(case[0])


def override_with(case, name, value):
    """The case's dictionary of overrides with `name` (an entry "x[i]" of a vector-valued name included) set to `value`."""
    ov = dict(overrides(case))
    base, idx = P.split_indexed_name(name)
    if idx is None:
        ov[base] = value
    else:
        lst = list(ov.get(base, P.DEFAULT_PARAMETERS[base]))
        lst[idx] = value
        ov[base] = lst
    return ov


@functools.lru_cache(maxsize=None)
def names(case):
    ov = overrides(case)
    return tuple(k for k in P.COLUMN_1M_DIRECTION_NAMES if _value(ov, k) != 0)


def theta(case, nm=None):
    ov = overrides(case)
    return np.array([_value(ov, k) for k in (names(case) if nm is None else nm)], dtype=np.float64)


def params(ft, case, ov=None):
    """(Microphysics1MParams, thermodynamics, Stokes cloud-liquid fall speed, Chen-2022 rain table, Chen-2022 ice tables), all five from ONE dictionary."""
    td = P.create_toml_dict(ft, overrides(case) if ov is None else ov)
    cr = P.Chen2022VelTypeRain(td)
    if case[1]:
        cr.b_rho = 0.6          # a table the Γ fit rejects: the general instantiation (run-time Γ)
    return P.Microphysics1MParams(td, **P1.options(case[0])), P.ThermodynamicsParameters(td), P.StokesRegimeVelType(td), cr, P.Chen2022VelTypeIce(td)


def tables_of(quints):
    return [(type(quints[0][k]) * len(quints))(*[q[k] for q in quints]) for k in range(5)]


def directions(ft, case, nm=None):
    """(the five structs, [d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice] tables of len(nm)): direction p is θ_p along name p, so a jvp column is S_·p."""
    nm = names(case) if nm is None else nm
    structs = params(ft, case)
    return structs, tables_of([P.column_parameter_direction_1m(structs[0], {k: float(t)}) for k, t in zip(nm, theta(case, nm))])


# ---- the reference --------------------------------------------------------------------------------------------------------------------------------
def oracle_column(case, ov, inv_dz, cols):
    import oracle_binding as oracle
    mp, tps, stokes, cr, ci = params("f64", case, ov)
    r = oracle.mp1m_column_tendencies_sedimentation(_abi.F64, mp.c, tps, stokes, cr, ci, mp.flags, inv_dz, *cols, nsub=0, float32_gates=False, nthreads=4)
    return np.stack([r[k] for k in OUT]), np.stack([np.array(r[k]) for k in PRECIP])


def fd_sensitivities(case, inv_dz, cols, nm, step):
    """(S [4, P, n], S_precip [2, P, n_col]) by central differences of the oracle with h = step·|θ_p|."""
    n_col, n_lev = cols[0].shape
    S, Sp = np.empty((4, len(nm), n_col * n_lev)), np.empty((2, len(nm), n_col))
    for p, (k, t) in enumerate(zip(nm, theta(case, nm))):
        h = step * abs(t)
        tp, tm = t + h, t - h
        (yp, pp), (ym, pm) = oracle_column(case, override_with(case, k, tp), inv_dz, cols), oracle_column(case, override_with(case, k, tm), inv_dz, cols)
        S[:, p] = (yp - ym) / (tp - tm) * t
        Sp[:, p] = (pp - pm) / (tp - tm) * t
    return S, Sp


@functools.lru_cache(maxsize=None)
def _reference(case, which, shape):
    import oracle_binding as oracle
    oracle.lib()
    inv_dz, cols = K1.columns(which, shape)
    nm = names(case)
    (S1, P1_), (S4, P4) = fd_sensitivities(case, inv_dz, cols, nm, 1e-6), fd_sensitivities(case, inv_dz, cols, nm, 4e-6)
    dis, disp = PC.row_error(S1, S4).max(axis=(0, 1)), PC.row_error(P1_, P4).max(axis=(0, 1))
    kept, keptp = dis <= AGREE, disp <= AGREE
    if shape == "n7":
        dead = np.array([not S1[:, p].any() and not S4[:, p].any() for p in range(len(nm))])
        deadp = np.array([not P1_[:, p].any() and not P4[:, p].any() for p in range(len(nm))])
    else:      # whether a name is dead is a property of the name, case and set, decided on the 840 points of n7 (module docstring)
        big = _reference(case, which, "n7")
        dead, deadp = big["dead"], big["deadp"]
    ref = dict(case=case, which=which, shape=shape, names=nm, n_col=cols[0].shape[0], n_lev=cols[0].shape[1], inv_dz=inv_dz, cols=cols, S=S1, Sp=P1_, S4=S4, Sp4=P4,
               kept=kept, keptp=keptp, dead=dead, deadp=deadp, worst=float(dis[kept].max(initial=0.0)), worstp=float(disp[keptp].max(initial=0.0)))
    for a in (S1, P1_, S4, P4, kept, keptp, dead, deadp, inv_dz, *cols):
        a.setflags(write=False)
    return ref


def reference_unchecked(case, which, shape):
    return _reference(tuple(case), which, shape)


def set_aside_shares(ref):
    return float((~ref["kept"]).mean()), float((~ref["keptp"]).mean())


def reference(case, which, shape):
    """The reference of (case, set, shape), computed once and shared read-only; prints the counts and asserts the 1 % condition where it is built."""
    ref = reference_unchecked(case, which, shape)
    pts, cls = set_aside_shares(ref)
    print(f"reference {case} {which} {shape}: {len(ref['names'])} names, set aside {int((~ref['kept']).sum())} of {ref['kept'].size} points, "
          f"{int((~ref['keptp']).sum())} of {ref['keptp'].size} columns; worst h-vs-4h on kept points {ref['worst']:.3g}, precipitation rows {ref['worstp']:.3g}; "
          f"live in a precipitation row: {int((~ref['deadp']).sum())}")
    assert pts <= MAX_SET_ASIDE and cls <= MAX_SET_ASIDE, (case, which, shape, pts, cls)
    return ref


# ---- the measure ----------------------------------------------------------------------------------------------------------------------------------
def _shares(S_ref, kept):
    A = np.abs(S_ref)[:, :, kept]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.nan_to_num(A / A.max(axis=1, keepdims=True)).max(axis=(0, 2))


def worst_errors(ref, S, Sp):
    """([P] worst row error of the tendencies over the kept points, [P] of the two precipitation rows over the kept columns)."""
    return PC.row_error(S, ref["S"])[:, :, ref["kept"]].max(axis=(0, 2)), PC.row_error(Sp, ref["Sp"])[:, :, ref["keptp"]].max(axis=(0, 2))


def assert_parity(ft, ref, S, Sp, what, report=True):
    """Every (row, parameter) of every kept point / column inside BOUND[ft]; every dead parameter exactly zero EVERYWHERE (NOT_STRUCTURALLY_DEAD excepted: the
    row bound only); Float64: the low-share columns also in their own scale.  S: [P, 4, n] (the jvp layout), Sp: [2, P, n_col]."""
    nm = ref["names"]
    S = np.asarray(S, dtype=np.float64).transpose(1, 0, 2)
    Sp = np.asarray(Sp, dtype=np.float64)
    e, ep = worst_errors(ref, S, Sp)
    if report:
        print(f"{what} {ft} {ref['case']} {ref['which']} {ref['shape']}: kept {int(ref['kept'].sum())}/{ref['kept'].size} points, "
              f"{int(ref['keptp'].sum())}/{ref['keptp'].size} columns; worst error — tendencies {e.max():.3g} ({nm[int(e.argmax())]}), precipitation {ep.max():.3g} "
              f"({nm[int(ep.argmax())]})")
    for p in np.nonzero(ref["dead"])[0]:
        if nm[p] not in NOT_STRUCTURALLY_DEAD:
            assert not S[:, p].any(), (what, nm[p], "dead in the reference, not exactly zero")
    for p in np.nonzero(ref["deadp"])[0]:
        if nm[p] not in NOT_STRUCTURALLY_DEAD:
            assert not Sp[:, p].any(), (what, nm[p], "dead in the reference's precipitation rows, not exactly zero")
    for p in np.nonzero(~(e < BOUND[ft]))[0]:
        raise AssertionError((what, "tendencies", nm[p], float(e[p])))
    for p in np.nonzero(~(ep < BOUND[ft]))[0]:
        raise AssertionError((what, "precipitation", nm[p], float(ep[p])))
    if ft == "f64":
        # LOW_SHARE (tests/param_cases.py): a live parameter whose largest row share stays below 0.02 is also held in the column's own scale, 1e-5·max_i |S^ref|
        # per row — on the rows whose column the reference itself resolves: its values at h and 4h agree there to 1e-6 of that scale, ten times inside the bound
        for rows, Sx, Sr, S4, kept, dead in ((4, S, ref["S"], ref["S4"], ref["kept"], ref["dead"]), (2, Sp, ref["Sp"], ref["Sp4"], ref["keptp"], ref["deadp"])):
            sh = _shares(Sr, kept)
            for p in [p for p in range(len(nm)) if not dead[p] and sh[p] < LOW_SHARE]:
                d = np.abs(Sx[:, p][:, kept] - Sr[:, p][:, kept]).max(axis=1)
                scale = np.abs(Sr[:, p][:, kept]).max(axis=1)
                resolved = (scale > 0) & (np.abs(S4[:, p][:, kept] - Sr[:, p][:, kept]).max(axis=1) <= 1e-6 * scale)      # (a row of zeros has no scale of its own)
                assert (d <= 1e-5 * scale)[resolved].all(), (what, nm[p], rows, d, scale)
    return e, ep


def grad_from_jvp(g, pbar, jv, jp):
    """[P] Σ ḡ·jvp + Σ p̄·ṗ (both precipitation rows) in float64, and [P] the sum of the terms' sizes.  jv: [P, 4, n], jp: [2, P, n_col], pbar: [2, n_col]."""
    g, jv = np.asarray(g, dtype=np.float64), np.asarray(jv, dtype=np.float64)
    t = (g[None] * jv).reshape(jv.shape[0], -1)
    tp = (np.asarray(pbar, dtype=np.float64)[:, None] * np.asarray(jp, dtype=np.float64)).transpose(1, 0, 2).reshape(jv.shape[0], -1)
    return t.sum(axis=1) + tp.sum(axis=1), np.abs(t).sum(axis=1) + np.abs(tp).sum(axis=1)


def cotangents(ref, seed=7):
    """(ḡ [4, n], p̄ [2, n_col]): every output weighed alike, ḡ_o = r / (largest |S^ref| of the row at the point), as tests/column_param_cases.py does."""
    rng = np.random.default_rng(seed)
    s, sp = np.abs(ref["S"]).max(axis=1), np.abs(ref["Sp"]).max(axis=1)
    r = rng.uniform(0.5, 1.0, s.shape) * rng.choice([-1.0, 1.0], s.shape)
    rp = rng.uniform(0.5, 1.0, sp.shape) * rng.choice([-1.0, 1.0], sp.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, r / s, 0.0), np.where(sp > 0, rp / sp, 0.0)


# ---- calls into the host build --------------------------------------------------------------------------------------------------------------------
def _flat(ft, a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=NPT[ft]) if a is not None else None


def _ptr(ft, a):
    return a.ctypes.data_as(C.POINTER(CT[ft])) if a is not None else None


def head(structs, override_flags=None):
    mp, tps, stokes, cr, ci = structs
    return (C.byref(mp.c), C.byref(tps), C.byref(stokes), C.byref(cr), C.byref(ci), C.c_uint32(mp.flags if override_flags is None else override_flags))


def _dirs(tables, lo=0, use=(True,) * 5):
    return [C.byref(t[lo]) if t is not None and u else None for t, u in zip(tables, use)]


def host_jvp(host, ft, structs, inv_dz, cols, tables, lo=0, ndir=None, kp=0, with_primal=True, override_flags=None, use=(True,) * 5, sentinel=-7.0):
    """(jvp [ndir, 4, n], jvp_precip [2, ndir, n_col], tendencies [4, n], precip [2, n_col], status ≥ 0: KIND of what ran) of the host build, for the directions
    lo … lo + ndir − 1 of the tables; more than CMX_PARAM_MAX_DIRS directions are several calls, as the wrappers make them."""
    n_col, n_lev = np.shape(cols[0])
    n = n_col * n_lev
    ndir = len(tables[0]) - lo if ndir is None else ndir
    if _abi.CMX_PARAM_MAX_DIRS < ndir <= len(tables[0]) - lo:
        parts = [host_jvp(host, ft, structs, inv_dz, cols, tables, lo + d0, min(_abi.CMX_PARAM_MAX_DIRS, ndir - d0), kp, with_primal and d0 == 0, override_flags, use,
                          sentinel) for d0 in range(0, ndir, _abi.CMX_PARAM_MAX_DIRS)]
        return (np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts], axis=1), parts[0][2], parts[0][3], min(q[4] for q in parts))
    x, dz = [_flat(ft, c) for c in cols], _flat(ft, inv_dz)
    jv, jp = np.full((max(ndir, 1), 4, n), sentinel, dtype=NPT[ft]), np.full((2, max(ndir, 1), n_col), sentinel, dtype=NPT[ft])
    tend, pr = np.full((4, n), sentinel, dtype=NPT[ft]), np.full((2, n_col), sentinel, dtype=NPT[ft])
    fn = getattr(host, f"host_mp1m_column_param_jvp_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head(structs, override_flags), C.c_int(kp), C.c_int64(n_col), C.c_int32(n_lev), _ptr(ft, dz), _arr(ft, x), C.c_int32(ndir), *_dirs(tables, lo, use),
            _arr(ft, [jv[d, o] for d in range(jv.shape[0]) for o in range(4)]), _arr(ft, list(jp[0])), _arr(ft, list(jp[1])),
            _arr(ft, list(tend)) if with_primal else None, _ptr(ft, pr[0]) if with_primal else None, _ptr(ft, pr[1]) if with_primal else None)
    return jv, jp, tend, pr, rc


def host_vjp(host, ft, structs, inv_dz, cols, g, pbar, tables, lo=0, ndir=None, kp=0, with_primal=False, override_flags=None, use=(True,) * 5, sentinel=-7.0):
    """(grad [ndir] float64, tendencies [4, n], precip [2, n_col], status) of the host build.  pbar: None or the pair (p̄_rai, p̄_sno), either may be None."""
    n_col, n_lev = np.shape(cols[0])
    n = n_col * n_lev
    ndir = len(tables[0]) - lo if ndir is None else ndir
    if _abi.CMX_PARAM_MAX_DIRS < ndir <= len(tables[0]) - lo:
        parts = [host_vjp(host, ft, structs, inv_dz, cols, g, pbar, tables, lo + d0, min(_abi.CMX_PARAM_MAX_DIRS, ndir - d0), kp, with_primal and d0 == 0,
                          override_flags, use, sentinel) for d0 in range(0, ndir, _abi.CMX_PARAM_MAX_DIRS)]
        return np.concatenate([q[0] for q in parts]), parts[0][1], parts[0][2], min(q[3] for q in parts)
    x, dz = [_flat(ft, c) for c in cols], _flat(ft, inv_dz)
    cot = [_flat(ft, a) for a in g] if g is not None else None
    pb = [_flat(ft, a) for a in pbar] if pbar is not None else [None, None]
    grad = np.full(max(ndir, 1), sentinel, dtype=np.float64)
    tend, pr = np.full((4, n), sentinel, dtype=NPT[ft]), np.full((2, n_col), sentinel, dtype=NPT[ft])
    fn = getattr(host, f"host_mp1m_column_param_vjp_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head(structs, override_flags), C.c_int(kp), C.c_int64(n_col), C.c_int32(n_lev), _ptr(ft, dz), _arr(ft, x), _arr(ft, cot) if cot is not None else None,
            _ptr(ft, pb[0]), _ptr(ft, pb[1]), C.c_int32(ndir), *_dirs(tables, lo, use), grad.ctypes.data_as(C.POINTER(C.c_double)),
            _arr(ft, list(tend)) if with_primal else None, _ptr(ft, pr[0]) if with_primal else None, _ptr(ft, pr[1]) if with_primal else None)
    return grad, tend, pr, rc
