"""The derivatives of the SB2006 column step with respect to the PARAMETERS on the device (cmx_sb2006_column_param_jvp_* / _param_vjp_*, include/cmx.h §(26);
cmx.column_param_jvp_2m, cmx.column_param_vjp_2m, cmx.autograd.column_tendencies_sedimentation_2m(…, theta=, names=)): the assertions of
tests/test_column_param_host.py through the C ABI and the kernels — same columns, names, reference, measure and 1 % condition (tests/column_param_cases.py) —
then what only the device has: the primal entry and the §22 entry to equal, the reduction, the statuses of the entry, graph capture, torch autograd.  No shape
is larger than 840 points."""
import numpy as np
import pytest
import torch

import column_param_cases as KC
import column_products_cases as CC  # noqa: F401
from jacobian_host_build import _build
from column_param_cases import CASE_IDS, CASES, MAIN_CASE, NAMES
import cmx
from cmx import _abi
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
FTS = ["f64", "f32"]
VEL = {"sb": cmx.SB2006VelType, "chen": cmx.Chen2022VelTypeRain, "chen_gen": cmx.Chen2022VelTypeRain}
NO_EXP = tuple(k for k in NAMES if k not in KC.EXPONENTS)
OTHER_CASES = [c for c in CASES if c != MAIN_CASE]
OTHER_IDS = [i for c, i in zip(CASES, CASE_IDS) if c != MAIN_CASE]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(a, ft, dev, shape=None):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a, dtype=np.float64)).to(DT[ft]).to(dev)
    return t.reshape(shape).contiguous() if shape is not None else t


def _eq(a, b):
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


class Setup:
    """The parameters of a case in one float type, the directions θ_p along each of `names`, and a reference's columns on the device."""
    def __init__(self, ft, ref, dev, names=NAMES, case=None):
        self.ft, self.ref, self.case, self.names = ft, ref, ref["case"] if case is None else case, names
        self.wr, self.tps, self.velp, self.stokes, tables = KC.directions(ft, self.case, names)
        self.dirs = [tuple(t[d] for t in tables) for d in range(len(names))]
        self.kw = dict(vel=VEL[self.case[1]], vel_params=self.velp, cloud_vel=self.stokes)
        self.shape = (ref["n_col"], ref["n_lev"])
        self.inv_dz = _t(ref["inv_dz"], ft, dev)
        self.cols = [_t(c, ft, dev, self.shape) for c in ref["cols"]]
        g, pbar = KC.cotangents(ref)
        self.cot, self.pbar = [_t(a, ft, dev, self.shape) for a in g], _t(pbar, ft, dev)

    def jvp(self, dirs=None, cols=None, inv_dz=None, **kw):
        return cmx.column_param_jvp_2m(self.wr, self.tps, self.inv_dz if inv_dz is None else inv_dz, *(self.cols if cols is None else cols),
                                       self.dirs if dirs is None else dirs, **kw, **self.kw)

    def vjp(self, cot="ref", pbar="ref", dirs=None, cols=None, **kw):
        return cmx.column_param_vjp_2m(self.wr, self.tps, self.inv_dz, *(self.cols if cols is None else cols), self.cot if isinstance(cot, str) else cot,
                                       self.pbar if isinstance(pbar, str) else pbar, self.dirs if dirs is None else dirs, **kw, **self.kw)

    def primal(self, cols=None):
        r = cmx.column_tendencies_sedimentation(self.wr, self.tps, self.inv_dz, *(self.cols if cols is None else cols), want_precip_flux=True, **self.kw)
        return torch.stack(list(r[:4])), r.precip_flux


def _np(r):
    return r.jvp.reshape(r.jvp.shape[0], 4, -1).cpu().numpy(), r.jvp_precip.cpu().numpy()


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except cmx.CmxStatusError as e:
        return e.status
    return 0


# ---- against the differenced oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("shape", ["n7", "n1", "n2", "n3"])
def test_the_main_case_in_full(dev, oracle, ft, shape):
    """limited, SB2006 fall speed, cloud sedimentation: every shape — tile boundaries inside columns, one level, two, two columns of three."""
    s = Setup(ft, KC.reference(MAIN_CASE, shape), dev)
    jv, jp = _np(s.jvp())
    KC.assert_parity(ft, s.ref, jv, jp, "device")


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", OTHER_CASES, ids=OTHER_IDS)
def test_the_other_cases(dev, oracle, ft, case):
    """One shape for limited / not-limited × {sb, chen, chen_gen} × cloud / no-cloud, with the exact zeros of the dead parameters; the gradient is the sum
    over the jvp columns — except the Float64 gradient of the general Chen-2022 instantiation, which is CMX_ERR_UNSUPPORTED (include/cmx.h §26)."""
    s = Setup(ft, KC.reference(case, "n7"), dev)
    jv, jp = _np(s.jvp())
    KC.assert_parity(ft, s.ref, jv, jp, "device")
    idx = {k: NAMES.index(k) for k in NAMES}
    if case[1] != "sb":
        for k in KC.NEW_NAMES[:3]:
            assert not jv[idx[k]].any() and not jp[idx[k]].any(), k
    if not case[2]:
        assert not jv[idx["gravitational_acceleration"]].any() and not jp[idx["gravitational_acceleration"]].any()
    for k in ("latent_heat_vaporization_at_reference", "temperature_triple_point", "thermal_conductivity_of_air", "condensation_evaporation_timescale"):
        assert not jp[idx[k]].any() and jv[idx[k]].any(), k
    if ft == "f64" and case[1] == "chen_gen":
        assert _status(s.vjp) == _abi.CMX_ERR_UNSUPPORTED
        return
    _assert_gradient(s, jv, jp, s.vjp().grad.cpu().numpy())


def _assert_gradient(s, jv, jp, grad):
    """grad[d] against Σ ḡ·jvp_d + Σ p̄·ṗ_d summed in float64 on the host from the jvp columns: the per-point sums differ by the rounding of a chain of at most
    eight fma in the float type, so |difference| ≤ 8 eps·Σ |terms| (the bound of the §22 gradient tests)."""
    g = torch.stack(s.cot).reshape(4, -1).cpu().numpy()
    want, size = KC.grad_from_jvp(g, s.pbar.cpu().numpy(), jv, jp)
    eps = np.finfo(KC.NPT[s.ft]).eps
    used = np.max(np.abs(grad - want) / np.where(size > 0, 8 * eps * size, 1.0))
    print(f"device {s.ft} {s.case}: gradient against the jvp columns, worst used fraction of 8 eps·Σ|terms| {used:.3g}")
    assert (np.abs(grad - want) <= 8 * eps * size).all() and ((size == 0) == (grad == 0)).all()


@pytest.mark.parametrize("ft", FTS)
def test_the_device_agrees_with_the_host_build(dev, oracle, ft):
    """Both lie within BOUND of the same reference, so they differ by less than 2·BOUND in the row measure (the host build has libm in the place of the
    hardware transcendental instructions: no bits are shared)."""
    s = Setup(ft, KC.reference(MAIN_CASE, "n7"), dev, names=NO_EXP)
    r = s.jvp(with_tendencies=True)
    jv, jp = _np(r)
    tables = [(type(s.dirs[0][k]) * len(s.dirs))(*[d[k] for d in s.dirs]) for k in range(4)]
    hv, hp, htend, hpr, rc = KC.host_jvp(_build("column_param_host"), ft, MAIN_CASE, (s.wr, s.tps, s.velp, s.stokes), s.ref["inv_dz"],
                                         s.ref["cols"], tables)
    assert rc >= 0
    kept, keptp = s.ref["kept"], s.ref["keptp"]
    e = KC.PC.row_error(jv.transpose(1, 0, 2), hv.transpose(1, 0, 2))[:, :, kept].max()
    ep = KC.PC.row_error(jp[None], hp[None])[:, :, keptp].max()
    print(f"{ft}: device against host build, worst row error {e:.3g}, precipitation {ep:.3g}")
    assert e < 2 * KC.BOUND[ft] and ep < 2 * KC.BOUND[ft]


# ---- bit identities ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", [MAIN_CASE, (False, "sb", False), (True, "chen", True), (False, "chen_gen", True)],
                         ids=["main", "notlimited-sb-nocloud", "limited-chen-cloud", "notlimited-chen_gen-cloud"])
def test_tendencies_and_precipitation_flux_are_the_column_entry(dev, oracle, ft, case):
    """Bit for bit, from both entries, when no direction touches an exponent."""
    s = Setup(ft, KC.reference(case, "n7"), dev, names=NO_EXP[:5] + KC.NEW_NAMES)
    want, wantp = s.primal()
    r = s.jvp(with_tendencies=True)
    assert _eq(r.tendencies, want) and _eq(r.precip_flux, wantp)
    if not (ft == "f64" and case[1] == "chen_gen"):
        v = s.vjp(with_tendencies=True)
        assert _eq(v.tendencies, want) and _eq(v.precip_flux, wantp)


@pytest.mark.parametrize("ft", FTS)
def test_a_column_does_not_depend_on_ndir_or_on_the_split(dev, oracle, ft):
    """1, KP, KP + 1 and 16 directions per call (KP = 4 Float32, 1 Float64: csrc/cmx_sb2006_column_param.hpp): the same bits; the gradient likewise, and
    bit-identical across two runs."""
    s = Setup(ft, KC.reference(MAIN_CASE, "n7"), dev, names=NAMES[:16])
    full = s.jvp()
    kp = 4 if ft == "f32" else 1
    for lo, nd in ((0, 1), (5, 1), (0, kp), (3, kp), (0, kp + 1), (7, kp + 1), (15, 1), (2, 14)):
        r = s.jvp(dirs=s.dirs[lo:lo + nd])
        assert _eq(r.jvp, full.jvp[lo:lo + nd]) and _eq(r.jvp_precip, full.jvp_precip[lo:lo + nd]), (lo, nd)
    g = s.vjp().grad
    assert _eq(g, s.vjp().grad)
    for lo, nd in ((0, 1), (0, kp), (1, kp + 1), (9, 3), (15, 1)):
        assert _eq(s.vjp(dirs=s.dirs[lo:lo + nd]).grad, g[lo:lo + nd]), (lo, nd)
    _assert_gradient(s, *_np(full), g.cpu().numpy())


@pytest.mark.parametrize("ft", FTS)
def test_results_do_not_depend_on_tile_boundaries(dev, oracle, ft):
    """The same columns at other places of the launch — a call on the columns [c0, c1) of the set moves every tile boundary of the halo kernel, which the
    parameter entry shares with the state products: the same bits.  n7: 7 levels, so a 255-point tile boundary falls inside a column, and 120 columns span
    several tiles."""
    s = Setup(ft, KC.reference(MAIN_CASE, "n7"), dev)
    full = s.jvp(with_tendencies=True)
    for c0, c1 in ((1, 120), (5, 77), (36, 38), (0, 37)):
        cut = lambda t: t[..., c0:c1, :].contiguous()  # noqa: E731
        r = s.jvp(cols=[cut(c) for c in s.cols], with_tendencies=True)
        assert _eq(r.jvp, cut(full.jvp)) and _eq(r.jvp_precip, full.jvp_precip[..., c0:c1]), (c0, c1)
        assert _eq(r.tendencies, cut(full.tendencies)) and _eq(r.precip_flux, full.precip_flux[c0:c1]), (c0, c1)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("cloud", [False, True])
def test_without_sedimentation_the_derivatives_are_the_pointwise_ones(dev, oracle, ft, cloud):
    """inv_dz ≡ 0: the flux terms multiply by an exact zero, and the jvp of the §22 names equals cmx_sb2006_warm_rain_param_jvp_* under == on states with finite
    flux tangents."""
    case = (True, "sb", cloud)
    names = tuple(k for k in KC.PC.NAMES if k not in KC.EXPONENTS)
    s = Setup(ft, KC.reference(case, "n7"), dev, names=names)
    r = s.jvp(inv_dz=torch.zeros_like(s.inv_dz))
    th = KC.theta(names)
    point = cmx.warm_rain_param_jvp_2m(s.wr, s.tps, *[c.reshape(-1) for c in s.cols], [{k: float(t)} for k, t in zip(names, th)])
    assert bool(torch.isfinite(r.jvp).all()) and bool(torch.isfinite(r.jvp_precip).all())
    assert bool((r.jvp.reshape(point.jvp.shape) == point.jvp).all())


# ---- the NaN rule, the statuses, graph capture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_the_nan_rule(dev, oracle, ft):
    s = Setup(ft, KC.reference(MAIN_CASE, "n2"), dev, names=NO_EXP[:3] + KC.NEW_NAMES)
    clean = s.jvp(with_tendencies=True)
    want_clean = s.primal()
    for j in range(7):
        bad = [c.clone() for c in s.cols]
        bad[j][5, 1] = float("nan")
        r = s.jvp(cols=bad, with_tendencies=True)
        want, wantp = s.primal(cols=bad)
        assert _eq(r.tendencies, want) and _eq(r.precip_flux, wantp), j
        assert bool(torch.isnan(r.jvp[:, :, 5, 1]).all()), j
        assert bool((torch.isnan(r.jvp[0]) == torch.isnan(want)).all()), j      # the flux NaN reaches the cell below exactly where it does in the primal
        keep = torch.ones(s.shape, dtype=torch.bool, device=dev)
        keep[5] = False
        assert _eq(r.jvp[:, :, keep], clean.jvp[:, :, keep]) and _eq(r.jvp_precip, clean.jvp_precip), j
        assert bool(torch.isnan(s.vjp(cols=bad).grad).all()), j
        bad = [c.clone() for c in s.cols]
        bad[j][5, 0] = float("nan")
        r = s.jvp(cols=bad)
        assert bool(torch.isnan(r.jvp_precip[:, 5]).all()) == (j in (0, 3, 4, 5, 6)), j
    cot = [c.clone() for c in s.cot]
    cot[1][3, 0] = float("nan")
    assert bool(torch.isnan(s.vjp(cot=cot).grad).all())
    assert _eq(s.primal()[0], want_clean[0])


def test_the_statuses_in_order(dev, oracle):
    s = Setup("f64", KC.reference(MAIN_CASE, "n3"), dev, names=NO_EXP[:3])
    BAD, UNS = _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED

    def bad_dirs(k, field, value, sub=None):
        d = [tuple(type(x).from_buffer_copy(x) for x in q) for q in s.dirs]
        setattr(getattr(d[1][k], sub) if sub else d[1][k], field, value)
        return d
    assert _status(s.jvp, dirs=bad_dirs(0, "condevap_tau_relax", float("inf"))) == BAD
    assert _status(s.jvp, dirs=bad_dirs(3, "grav", float("nan"))) == BAD
    assert _status(s.jvp, dirs=bad_dirs(2, "b_rho", 1e-3, "chen2022")) == UNS and _status(s.vjp, dirs=bad_dirs(2, "b_rho", 1e-3, "chen2022")) == UNS
    # the flags come before the directions, a non-finite component before the Chen-2022 table
    d = bad_dirs(2, "b_rho", 1e-3, "chen2022")
    d[0][1].cp_v = float("inf")
    assert _status(s.jvp, dirs=d) == BAD
    # the aliasing refusal: a cotangent column that is a state column's storage is fine (both are inputs); an output may not be an input — through the raw entry
    import ctypes as C
    from cmx import _lib
    from cmx.bulk_tendencies import _column_products_head, _table, _ptr
    ref, fam, keep, head = _column_products_head(s.wr, s.tps, s.inv_dz, s.cols, VEL["sb"], s.velp, s.stokes)
    tables = [(type(s.dirs[0][k]) * 3)(*[q[k] for q in s.dirs]) for k in range(4)]
    out = torch.empty((3, 4, *s.shape), dtype=torch.float64, device=dev)
    outp = torch.empty((3, s.shape[0]), dtype=torch.float64, device=dev)

    def raw(jvp_cols, precip_cols):
        fn = getattr(_lib.lib(), "cmx_sb2006_column_param_jvp_f64")
        with torch.cuda.device(dev):
            return fn(*head, 3, *[C.byref(t[0]) for t in tables], _table(jvp_cols), _table(precip_cols), None, None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    cols = [out[d, o] for d in range(3) for o in range(4)]
    assert raw(cols, list(outp)) == 0
    assert raw([s.cols[3]] + cols[1:], list(outp)) == BAD and raw(cols, [s.inv_dz] + list(outp)[1:]) == BAD
    assert raw([None] * 12, [None] * 3) == BAD                       # no output at all
    torch.cuda.synchronize()
    # n_col = 0: CMX_OK; the gradient entry writes zeros
    empty = [c[:0].contiguous() for c in s.cols]
    assert s.jvp(cols=empty).jvp.shape == (3, 4, 0, 3)
    g = cmx.column_param_vjp_2m(s.wr, s.tps, s.inv_dz, *empty, [None] * 4, None, s.dirs, **s.kw).grad
    assert g.shape == (3,) and not bool(g.any())


@pytest.mark.parametrize("ft", FTS)
def test_a_captured_call_replays_bit_identically(dev, oracle, ft):
    s = Setup(ft, KC.reference(MAIN_CASE, "n7"), dev, names=NO_EXP[:2] + KC.NEW_NAMES)
    eager_j, eager_g = s.jvp(), s.vjp()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rj, rg = s.jvp(), s.vjp()
    rj.jvp.fill_(float("nan")), rj.jvp_precip.fill_(float("nan")), rg.grad.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert _eq(rj.jvp, eager_j.jvp) and _eq(rj.jvp_precip, eager_j.jvp_precip) and _eq(rg.grad, eager_g.grad)


# ---- torch autograd ---------------------------------------------------------------------------------------------------------------------------------
AG_NAMES = ("SB2006_raindrops_terminal_velocity_coeff_aR", "SB2006_raindrops_terminal_velocity_coeff_cR", "gravitational_acceleration", "density_liquid_water",
            "SB2006_collection_kernel_coeff_kcr", "latent_heat_vaporization_at_reference")


@pytest.mark.parametrize("ft", FTS)
def test_precipitation_loss_reaches_theta(dev, oracle, ft):
    """theta.grad of precip_flux.sum() equals column_param_vjp_2m and matches the oracle's difference quotient to BOUND in the precipitation row's scale; forward
    mode agrees with the jvp entry; without theta the function returns the bits it returned before."""
    ref = KC.reference(MAIN_CASE, "n7")
    s = Setup(ft, ref, dev, names=AG_NAMES)
    th0 = KC.theta(AG_NAMES)
    theta = torch.tensor(th0, dtype=torch.float64, requires_grad=True)
    args = (s.wr, s.tps, s.inv_dz, *s.cols)
    out = cmx.autograd.column_tendencies_sedimentation_2m(*args, theta=theta, names=AG_NAMES, **s.kw)
    plain = cmx.autograd.column_tendencies_sedimentation_2m(*args, **s.kw)
    want, wantp = s.primal()
    for o in range(4):
        assert _eq(out[o], want[o]) and _eq(plain[o], want[o])
    assert _eq(out[4], wantp) and _eq(plain[4], wantp)
    out[4].sum().backward()
    ones = torch.ones_like(wantp)
    direct = cmx.column_param_vjp_2m(*args, [None] * 4, ones, AG_NAMES, **s.kw).grad.cpu()
    assert _eq(theta.grad, direct)
    # Σ_col ∂precip/∂θ_p·θ_p against the reference's S_precip summed over the kept columns, in the row's scale s_p per column
    idx = [NAMES.index(k) for k in AG_NAMES]
    only_kept = _t(ref["keptp"].astype(np.float64), ft, dev)
    gk = cmx.column_param_vjp_2m(*args, [None] * 4, only_kept, AG_NAMES, **s.kw).grad.cpu().numpy() * th0
    Sp = ref["Sp"][0][:, ref["keptp"]]
    scale = np.abs(Sp).max(axis=0).sum()
    err = np.abs(gk - Sp[idx].sum(axis=1)) / scale
    print(f"{ft}: theta.grad of the precipitation loss against the oracle's difference quotient, worst {err.max():.3g} of Σ s_p")
    assert (err < KC.BOUND[ft]).all(), err
    # forward mode: a tangent on theta
    import torch.autograd.forward_ad as fwd
    tvec = torch.tensor(th0 * np.array([1.0, -0.5, 0.25, 2.0, 0.0, 1.5]), dtype=torch.float64)
    with fwd.dual_level():
        o = cmx.autograd.column_tendencies_sedimentation_2m(*args, theta=fwd.make_dual(theta.detach(), tvec), names=AG_NAMES, **s.kw)
        tang = [fwd.unpack_dual(x).tangent for x in o]
    r = s.jvp(dirs=[dict(zip(AG_NAMES, tvec.tolist()))])
    for q in range(4):
        assert _eq(tang[q], r.jvp[0, q])
    assert _eq(tang[4], r.jvp_precip[0])


def test_a_fall_speed_struct_that_the_dictionary_does_not_build_is_refused(dev, oracle):
    s = Setup("f64", KC.reference(MAIN_CASE, "n3"), dev, names=AG_NAMES)
    theta = torch.tensor(KC.theta(AG_NAMES), dtype=torch.float64, requires_grad=True)
    velp = P.rain_vel_params("f64")
    velp.sb2006.aR = 9.0
    with pytest.raises(ValueError, match="vel_params"):
        cmx.autograd.column_tendencies_sedimentation_2m(s.wr, s.tps, s.inv_dz, *s.cols, theta=theta, names=AG_NAMES, vel_params=velp, cloud_vel=s.stokes)
    with pytest.raises(ValueError, match="names"):
        cmx.autograd.column_tendencies_sedimentation_2m(s.wr, s.tps, s.inv_dz, *s.cols, theta=theta[:1], names=("Chen2022_table_B1_coeff_b_rho",), **s.kw)


def test_the_public_names():
    assert cmx.ColumnParamJvp2M._fields == ("jvp", "jvp_precip", "tendencies", "precip_flux")
    assert cmx.ColumnParamVjp2M._fields == ("grad", "tendencies", "precip_flux", "wrt")
    assert callable(cmx.column_param_jvp_2m) and callable(cmx.column_param_vjp_2m)
    assert set(P.WARM_RAIN_2M_DIRECTION_FIELDS) < set(P.COLUMN_2M_DIRECTION_FIELDS) and set(KC.NEW_NAMES) <= set(P.COLUMN_2M_DIRECTION_FIELDS)
