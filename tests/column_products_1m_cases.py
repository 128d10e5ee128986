"""What tests/test_column_products_1m_host.py and tests/test_column_products_1m_gpu.py share: the columns, the finite-difference reference of the Float64
ORACLE's 1-moment column step (oracle_binding.mp1m_column_tendencies_sedimentation, nsub = 0), the measure, and the ctypes calls into the host build
tests/native/column_products_1m_host.cpp.  Modelled on tests/column_products_cases.py (the SB2006 column step); what differs is the scheme — four falling
species, two precipitation fluxes — not the recipe.

STATES.  jacobian_1m_cases.states(oracle, which) for which in ("cold", "warm") with its default n and seed (all four species present, T at least 0.5 K from
T_freeze), arranged into columns, level 0 lowest, at the offsets and shapes of the 2-moment file; q_rai = 0 where the flat index % 13 == 7 and q_sno = 0
where it is % 13 == 3: cells that receive a flux and send none.  Shapes, the smallest at which a 255-point tile can go wrong
(cmx_mp1m_column_products.hip: one point per lane, a workgroup owns 255 points):
    n7  120 columns of 7 levels = 840 points at offset 0: the tile boundaries 255, 510 and 765 fall inside columns, at levels 3, 6 and 2
    n1  64 columns of 1 level at offset 840: every cell is top and surface     n2  32 × 2 at 904     n3  2 × 3 at 968
inv_dz = 1/(40 + 35k + 11(k mod 3)).

CASES.  The parameter cases of jacobian_1m_cases.CASES — default (the compile-time instantiation), alt and exponents (the run-time-flags one) — and default
with a Chen-2022 rain table of b_ρ = 0.6, which the Γ fit rejects (the general instantiation, run-time Γ).

REFERENCE.  J v by central differences of the oracle ALONG v, without assembling J: y_ref = (f(x + t v) − f(x − t v)) / 2t with v_j = r_j·x_j, r drawn as in
the 2-moment file; t = 1e-6, and 4e-6 for the set-aside criterion.

MEASURE: the input-scaled stencil measure of tests/column_products_cases.py, unchanged:
    s'_i = max over both blocks of |J^ref_ij|·|x_j|      (from the REFERENCE alone; the two blocks by differencing one input at the even / the odd levels)
    R_i  = Σ_j |r_j| over the own level and the level above (inputs with x_j = 0 carry no tangent and are not counted)
    |y_i − y_i^ref| < B·s'_i·R_i,      B = jacobian_cases.BOUND (1e-5 Float64, 1e-3 Float32)
Each of the two precipitation fluxes is a row of its own, with the six entries of level 0.  Cotangents weigh every output alike: ḡ_q = r'_q / s'_q,
p̄ = r'_p / s'_p.  The adjoint identity is summed over each whole column, with both precipitation terms, at 2B.
A point is SET ASIDE only by a criterion of the reference: y_ref at t and at 4t disagree by more than AGREE = 2e-6 in this measure; a column is set aside for
the adjoint identity if one of its points or one of its precipitation rows is.  At most MAX_SET_ASIDE (1 %) of the points and of the columns of a set may be
set aside (`checked`; asserted in the host test).  With exactly these states and this recipe: cold n7, every case, 1 of 840 points (0.12 %) and 1 of 120
columns (0.83 %); warm n7 and n1 / n2 / n3 none; no precipitation row; worst t-vs-4t value on kept points 8.6e-8."""
import ctypes as C
import functools

import numpy as np

import jacobian_cases as JC
import jacobian_1m_cases as J1
from jacobian_host_build import CT, NPT, _arr, _same_bits, host_fixture  # noqa: F401
from cmx import _abi
from cmx import parameters as P

host = host_fixture("column_products_1m_host")
BOUND, AGREE, MAX_SET_ASIDE = JC.BOUND, JC.AGREE, JC.MAX_SET_ASIDE
WRT, OUT = J1.WRT, J1.OUT
PRECIP = ("precip_rai", "precip_sno")
CASES = [(p, False) for p in J1.CASES] + [("default", True)]
CASE_IDS = [f"{c[0]}{'-general_gamma' if c[1] else ''}" for c in CASES]
MAIN_CASE = ("default", False)
WHICH = ("cold", "warm")
# what the host build returns: bit 0 the default-options instantiation, bit 1 the general Γ of the Chen-2022 rain table
KIND = {("default", False): 1, ("alt", False): 0, ("exponents", False): 0, ("default", True): 3}
SHAPES = {"n7": (120, 7), "n1": (64, 1), "n2": (32, 2), "n3": (2, 3)}
_OFFSET = {"n7": 0, "n1": 840, "n2": 904, "n3": 968}


# ---- parameters -----------------------------------------------------------------------------------------------------------------------------------
def chen_rain(ft, general):
    """The Chen-2022 rain table; general: b_ρ = 0.6, a table the Γ fit rejects (the general instantiation, run-time Γ)."""
    v = P.Chen2022VelTypeRain(ft)
    if general:
        v.b_rho = 0.6
    return v


def params(ft, case):
    """(Microphysics1MParams, thermodynamics, Stokes cloud-liquid fall speed, Chen-2022 rain table, Chen-2022 ice tables) of a case in one float type."""
    return J1.params(ft, case[0]), P.ThermodynamicsParameters(ft), P.StokesRegimeVelType(ft), chen_rain(ft, case[1]), P.Chen2022VelTypeIce(ft)


# ---- columns --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _states(which):
    import oracle_binding as oracle
    oracle.lib()
    return J1.states(oracle, which)


def columns(which, shape):
    """(inv_dz [n_lev], the seven state columns, each (n_col, n_lev), Float64) of a set and a shape."""
    n_col, n_lev = SHAPES[shape]
    lo, n = _OFFSET[shape], n_col * n_lev
    cols = [np.array(c[lo:lo + n], dtype=np.float64).reshape(n_col, n_lev) for c in _states(which)]
    flat = np.arange(lo, lo + n).reshape(n_col, n_lev)
    cols[5][flat % 13 == 7] = 0.0
    cols[6][flat % 13 == 3] = 0.0
    inv_dz = 1.0 / (40.0 + 35.0 * np.arange(n_lev) + 11.0 * (np.arange(n_lev) % 3))
    return inv_dz, cols


def oracle_column(oracle, case, inv_dz, cols):
    """([4, n] tendencies, [2, n_col] precipitation fluxes of rain and snow) of the Float64 oracle's column step, Instantaneous mode."""
    mp, tps, stokes, cr, ci = params("f64", case)
    r = oracle.mp1m_column_tendencies_sedimentation(_abi.F64, mp.c, tps, stokes, cr, ci, mp.flags, inv_dz, *cols, nsub=0, float32_gates=False, nthreads=4)
    return np.stack([r[k] for k in OUT]), np.stack([np.array(r[k]) for k in PRECIP])


# ---- the reference --------------------------------------------------------------------------------------------------------------------------------
def _row_scales(f, inv_dz, cols, step=1e-6):
    """(s' [4, n], s'_p [2, n_col]) of the module docstring: one input differenced at the even, then at the odd levels, gives the own-level and the
    level-above entry of every row separately (the block Jacobian is upper bidiagonal)."""
    n_col, n_lev = cols[0].shape
    lev = np.arange(n_lev)
    s, sp = np.zeros((4, n_col, n_lev)), np.zeros((2, n_col))
    for j in range(6):
        x = cols[j + 1]
        for parity in range(min(2, n_lev)):
            on = (lev % 2 == parity)[None, :]
            h = np.where(on, step * np.abs(x), 0.0)
            xp, xm = x + h, x - h
            (fp, pp), (fm, pm) = f(cols[:j + 1] + [xp] + cols[j + 2:]), f(cols[:j + 1] + [xm] + cols[j + 2:])
            d = (fp - fm).reshape(4, n_col, n_lev)
            dx = xp - xm
            with np.errstate(divide="ignore", invalid="ignore"):
                own = np.where(dx != 0, d / dx[None], 0.0) * np.abs(x)[None]                        # rows of the perturbed levels
                up = np.zeros_like(d)
                up[:, :, :-1] = np.where(dx[:, 1:] != 0, d[:, :, :-1] / dx[None, :, 1:], 0.0) * np.abs(x[:, 1:])[None]      # rows below a perturbed level
                if parity == 0:
                    sp = np.maximum(sp, np.abs(np.where(dx[:, 0] != 0, (pp - pm) / dx[None, :, 0], 0.0) * x[None, :, 0]))
            s = np.maximum(s, np.where(on[None], np.abs(own), np.abs(up)))
    return s.reshape(4, -1), sp


@functools.lru_cache(maxsize=None)
def _reference(case, which, shape, seed=5):
    import oracle_binding as oracle
    oracle.lib()
    inv_dz, cols = columns(which, shape)
    n_col, n_lev = cols[0].shape
    f = lambda c: oracle_column(oracle, case, inv_dz, c)  # noqa: E731
    s, sp = _row_scales(f, inv_dz, cols)
    x = np.stack(cols[1:])                                                   # [6, n_col, n_lev]
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.5, 1.0, x.shape) * rng.choice([-1.0, 1.0], x.shape)
    rq = rng.uniform(0.5, 1.0, (4, n_col * n_lev)) * rng.choice([-1.0, 1.0], (4, n_col * n_lev))
    rp = rng.uniform(0.5, 1.0, (2, n_col)) * rng.choice([-1.0, 1.0], (2, n_col))
    v = r * x
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(s > 0, rq / s, 0.0)
        pbar = np.where(sp > 0, rp / sp, 0.0)
    rl = (np.abs(r) * (x != 0)).sum(axis=0)                                  # Σ_j |r_j| per point
    R = rl.copy()
    R[:, :-1] += rl[:, 1:]
    R, Rp = R.reshape(-1), rl[:, 0]

    def along(t):
        (fp, pp), (fm, pm) = f([cols[0]] + list(x + t * v)), f([cols[0]] + list(x - t * v))
        return (fp - fm) / (2 * t), (pp - pm) / (2 * t)
    (y1, p1), (y4, p4) = along(1e-6), along(4e-6)

    def frac(err, lim):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(lim > 0, err / lim, np.where(err == 0, 0.0, np.inf))
    dis_all = frac(np.abs(y1 - y4), s * R[None])
    dis = dis_all.max(axis=0)
    disp = frac(np.abs(p1 - p4), sp * Rp[None])
    kept = dis <= AGREE
    keptp = disp <= AGREE                                                    # [2, n_col]
    keptc = kept.reshape(n_col, n_lev).all(axis=1) & keptp.all(axis=0)
    worst_kept = float(max(dis[kept].max() if kept.any() else 0.0, disp[keptp].max() if keptp.any() else 0.0))
    ref = dict(case=case, which=which, shape=shape, n_col=n_col, n_lev=n_lev, inv_dz=inv_dz, cols=cols, v=list(v), g=list(g), pbar=pbar, s=s, sp=sp, R=R, Rp=Rp,
               y=y1, yp=p1, kept=kept, keptp=keptp, keptc=keptc, worst=float(max(dis.max(), disp.max())), worst_kept=worst_kept)
    for a in (inv_dz, *cols, *ref["v"], *ref["g"], pbar, s, sp, R, Rp, y1, p1, kept, keptp, keptc):
        a.setflags(write=False)
    return ref


def reference_unchecked(case, which, shape):
    return _reference(tuple(case), which, shape)


def set_aside_shares(ref):
    """(share of the points, share of the columns) that the reference's criterion sets aside."""
    return float((~ref["kept"]).mean()), float((~ref["keptc"]).mean())


def checked(ref):
    """The 1 % condition on a reference."""
    pts, cls = set_aside_shares(ref)
    assert pts <= MAX_SET_ASIDE and cls <= MAX_SET_ASIDE, (ref["case"], ref["which"], ref["shape"], pts, cls, ref["worst"])
    return ref


def reference(case, which, shape):
    """The reference of (case, set, shape), computed once and shared read-only; asserts the 1 % condition."""
    return checked(reference_unchecked(case, which, shape))


# ---- the measure ----------------------------------------------------------------------------------------------------------------------------------
def _worst(err, lim, kept):
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(lim > 0, err / lim, np.where(err == 0, 0.0, np.inf))
    f = np.where(np.isfinite(f), f, np.inf)
    f = f[..., kept] if kept.ndim == 1 else f[kept]
    return float(f.max()) if f.size else 0.0


def jvp_fractions(ref, y, yp, bound):
    """The worst used fraction of the bound over the kept points: (J v, the two ṗ rows together)."""
    y, yp = np.asarray(y, dtype=np.float64), np.asarray(yp, dtype=np.float64)
    return (_worst(np.abs(y - ref["y"]), bound * ref["s"] * ref["R"][None], ref["kept"]),
            _worst(np.abs(yp - ref["yp"]), bound * ref["sp"] * ref["Rp"][None], ref["keptp"]))


def adjoint_fraction(ref, y, yp, grad, bound):
    """The worst used fraction of the 2B bound of the adjoint identity over the kept columns: y = J v, yp = (ṗ_rai, ṗ_sno), grad = Jᵀḡ of the code under test
    on the reference's v, ḡ, p̄."""
    n_col, n_lev = ref["n_col"], ref["n_lev"]
    y, yp, grad = np.asarray(y, dtype=np.float64), np.asarray(yp, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    g, v = np.stack(ref["g"]), np.stack(ref["v"]).reshape(6, -1)
    lhs = (g * y).sum(axis=0).reshape(n_col, n_lev).sum(axis=1) + (ref["pbar"] * yp).sum(axis=0)
    rhs = (grad * v).sum(axis=0).reshape(n_col, n_lev).sum(axis=1)
    lim = 2 * bound * (((np.abs(g) * ref["s"]).sum(axis=0) * ref["R"]).reshape(n_col, n_lev).sum(axis=1) + (np.abs(ref["pbar"]) * ref["sp"] * ref["Rp"][None]).sum(axis=0))
    return _worst(np.abs(lhs - rhs), lim, ref["keptc"])


def assert_products(ft, ref, y, yp, grad, what, report=True):
    fy, fp = jvp_fractions(ref, y, yp, BOUND[ft])
    fa = adjoint_fraction(ref, y, yp, grad, BOUND[ft])
    if report:
        print(f"{what} {ft} {ref['case']} {ref['which']} {ref['shape']}: kept {int(ref['kept'].sum())}/{ref['kept'].size} points, "
              f"{int(ref['keptc'].sum())}/{ref['keptc'].size} columns, t-vs-4t {ref['worst']:.3g} (kept {ref['worst_kept']:.3g}); worst used fraction of the bound — "
              f"J v {fy:.3g}, precipitation {fp:.3g}, adjoint identity {fa:.3g}")
    assert fy < 1.0, (what, "J v", fy)
    assert fp < 1.0, (what, "precip", fp)
    assert fa < 1.0, (what, "adjoint", fa)
    return fy, fp, fa


# ---- calls into the host build --------------------------------------------------------------------------------------------------------------------
def _flat(ft, a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=NPT[ft]) if a is not None else None


def _ptr(ft, a):
    return a.ctypes.data_as(C.POINTER(CT[ft])) if a is not None else None


def _head(ft, case, override_flags=None):
    mp, tps, stokes, cr, ci = keep = params(ft, case)
    return keep, (C.byref(mp.c), C.byref(tps), C.byref(stokes), C.byref(cr), C.byref(ci), C.c_uint32(mp.flags if override_flags is None else override_flags))


def host_jvp(host, ft, case, inv_dz, cols, tangents, want=(True,) * 4, want_precip=(True, True), with_primal=True, override_flags=None, sentinel=-7.0):
    """(jvp [4, n], jvp_precip [2, n_col], tendencies [4, n], precip [2, n_col], status ≥ 0: KIND of what ran) of the host build.  tangents: six arrays or
    None, or None for a NULL table.  Buffers that are not requested keep the sentinel."""
    n_col, n_lev = np.shape(cols[0])
    n = n_col * n_lev
    x, dz = [_flat(ft, c) for c in cols], _flat(ft, inv_dz)
    t = [_flat(ft, a) for a in tangents] if tangents is not None else None
    jv, tend = np.full((4, n), sentinel, dtype=NPT[ft]), np.full((4, n), sentinel, dtype=NPT[ft])
    jp, pr = np.full((2, n_col), sentinel, dtype=NPT[ft]), np.full((2, n_col), sentinel, dtype=NPT[ft])
    keep, head = _head(ft, case, override_flags)
    fn = getattr(host, f"host_mp1m_column_jvp_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_int64(n_col), C.c_int32(n_lev), _ptr(ft, dz), _arr(ft, x), _arr(ft, t) if t is not None else None,
            _arr(ft, [jv[q] if want[q] else None for q in range(4)]), _ptr(ft, jp[0]) if want_precip[0] else None, _ptr(ft, jp[1]) if want_precip[1] else None,
            _arr(ft, list(tend)) if with_primal else None, _ptr(ft, pr[0]) if with_primal else None, _ptr(ft, pr[1]) if with_primal else None)
    return jv, jp, tend, pr, rc


def host_vjp(host, ft, case, inv_dz, cols, cotangents, cot_precip, want=(True,) * 6, with_primal=True, k=0, override_flags=None, sentinel=-7.0):
    """(grad [6, n], tendencies [4, n], precip [2, n_col], status) of the host build.  cotangents: four arrays or None, or None for a NULL table; cot_precip:
    None or the pair (p̄_rai, p̄_sno), either of which may be None."""
    n_col, n_lev = np.shape(cols[0])
    n = n_col * n_lev
    x, dz = [_flat(ft, c) for c in cols], _flat(ft, inv_dz)
    g = [_flat(ft, a) for a in cotangents] if cotangents is not None else None
    pb = [_flat(ft, a) for a in cot_precip] if cot_precip is not None else [None, None]
    grad, tend, pr = np.full((6, n), sentinel, dtype=NPT[ft]), np.full((4, n), sentinel, dtype=NPT[ft]), np.full((2, n_col), sentinel, dtype=NPT[ft])
    keep, head = _head(ft, case, override_flags)
    fn = getattr(host, f"host_mp1m_column_vjp_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_int(k), C.c_int64(n_col), C.c_int32(n_lev), _ptr(ft, dz), _arr(ft, x), _arr(ft, g) if g is not None else None, _ptr(ft, pb[0]), _ptr(ft, pb[1]),
            _arr(ft, [grad[j] if want[j] else None for j in range(6)]), _arr(ft, list(tend)) if with_primal else None,
            _ptr(ft, pr[0]) if with_primal else None, _ptr(ft, pr[1]) if with_primal else None)
    return grad, tend, pr, rc


def host_plain(host, ft, case, inv_dz, cols):
    """([4, n] tendencies, [2, n_col] precipitation fluxes, status) of the PLAIN instantiation in the host build: the operations of the primal kernel."""
    n_col, n_lev = np.shape(cols[0])
    x, dz = [_flat(ft, c) for c in cols], _flat(ft, inv_dz)
    y, pr = np.empty((4, n_col * n_lev), dtype=NPT[ft]), np.empty((2, n_col), dtype=NPT[ft])
    keep, head = _head(ft, case)
    fn = getattr(host, f"host_mp1m_column_plain_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_int64(n_col), C.c_int32(n_lev), _ptr(ft, dz), _arr(ft, x), _arr(ft, list(y)), _ptr(ft, pr[0]), _ptr(ft, pr[1]))
    return y, pr, rc
