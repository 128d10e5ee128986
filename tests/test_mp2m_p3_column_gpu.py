"""GPU tests of the 2M + P3 column step (cmx_mp2m_p3_column_tendencies_sedimentation_*): against its parts (the library's own pointwise
entries, bit for bit, + the upwind divergence in torch), against the oracle composition of tests/p3_column_ref.py, on the smallest shapes
at which the sedimentation kernel can go wrong and on misaligned twins, the warm start, the NaN policy, and graph capture.

The flux step is the host model's scheme, not the reference's ("parity unpinned"): its oracle is the formula restated in p3_column_ref."""
import numpy as np
import pytest
import torch

import p3_column_ref as R
import parity
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}
NAMES = R.NAMES
FIELDS = NAMES + ("log_lambda", "v_ice_n", "v_ice_m", "precip_rai", "precip_ice")
# species → (state column, which fall speed); the cloud pair sediments only with cloud_vel
SED = {"dq_rai_dt": ("q_rai", "w_m"), "dn_rai_dt": ("n_rai", "w_n"), "dq_ice_dt": ("q_ice", "v_m"), "dn_ice_dt": ("n_ice", "v_n"),
       "dq_rim_dt": ("q_rim", "v_m"), "db_rim_dt": ("b_rim", "v_m"), "dq_lcl_dt": ("q_lcl", "c_m"), "dn_lcl_dt": ("n_lcl", "c_n")}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _np64(t):
    return t.cpu().numpy().astype(np.float64)


def _biteq(a, b):
    """Equal bit for bit (−Inf, NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def _vel(name):
    import cmx
    return cmx.SB2006VelType if name == "sb" else cmx.Chen2022VelTypeRain


def _case(dev, ft, n_col, n_lev, seed, limited=True):
    s = R.states(n_col, n_lev, seed=seed, f32_safe=(ft == "f32"))
    d = {k: torch.from_numpy(v).to(DT[ft]).to(dev) for k, v in s.items()}
    dz = torch.from_numpy(R.inv_dz(n_lev, seed=seed)).to(DT[ft]).to(dev)
    return d, dz, P.Microphysics2MParams(ft, with_ice=True, is_limited=limited), P.ThermodynamicsParameters(ft)


def _step(d, dz, mp, tps, vel, cloud, **kw):
    import cmx
    ft = "f32" if dz.dtype == torch.float32 else "f64"
    return cmx.column_tendencies_sedimentation_2m_p3(mp, tps, dz, *[d[k] for k in R.IN_NAMES], vel=_vel(vel),
                                                     cloud_vel=P.StokesRegimeVelType(ft) if cloud else None, want_precip_flux=True, **kw)


def _check_against_parts(got, d, dz, mp, tps, ft, limited, vel, cloud, guess=None, shift=None, brent_iters=0):
    """Point 1 of the issue: log λ and the ice speeds are the shape + fall-speed entry's bits; a column that does not sediment is the pointwise
    2M + P3 entry's bits; a sedimenting column is pointwise tendency + torch divergence within (8 | 64)·eps·(|tend| + (F_up + F)·inv_dz/ρ) + tiny."""
    import cmx
    sh = d["rho"].shape
    flat = {k: v.reshape(-1) for k, v in d.items()}
    rho = flat["rho"]
    sv = cmx.p3_shape_and_terminal_velocities(P.ParametersP3(ft), P.Chen2022VelTypeIce(ft), rho, rho * flat["q_ice"], rho * flat["n_ice"], rho * flat["q_rim"],
                                              rho * flat["b_rim"], log_lambda_guess=None if guess is None else guess.reshape(-1), brent_iters=brent_iters,
                                              p=1e-6, quad=mp.ice.c.quad)
    assert _biteq(got.log_lambda.reshape(-1), sv.log_lambda) and _biteq(got.v_ice_n.reshape(-1), sv.v_n) and _biteq(got.v_ice_m.reshape(-1), sv.v_m)
    ll0 = torch.where(torch.isfinite(sv.log_lambda), sv.log_lambda, torch.zeros_like(sv.log_lambda))
    pt = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), mp, tps, *[flat[k] for k in R.IN_NAMES], ll0,
                                          None if shift is None else shift.reshape(-1))
    warm = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), P.Microphysics2MParams(ft, is_limited=limited), tps,
                                            *[flat[k] for k in R.IN_NAMES[:7]], vel=_vel(vel))
    cl = {k: torch.clamp(v, min=0) for k, v in d.items()}
    w = {"w_n": warm.vt_rai_n.reshape(sh), "w_m": warm.vt_rai_m.reshape(sh), "v_n": got.v_ice_n, "v_m": got.v_ice_m}
    if cloud:
        cv = cmx.cloud_terminal_velocity(mp.warm_rain.c.seifert_beheng.pdf_c, P.StokesRegimeVelType(ft), cl["q_lcl"].reshape(-1), cl["rho"].reshape(-1),
                                         (cl["rho"] * cl["n_lcl"]).reshape(-1))
        w["c_n"], w["c_m"] = cv.vt_n.reshape(sh), cv.vt_m.reshape(sh)
    eps, tiny = torch.finfo(DT[ft]).eps, torch.finfo(DT[ft]).tiny
    k_eps = (8 if ft == "f32" else 64) * eps
    g = dz[None, :] / cl["rho"]
    for name in NAMES:
        tend = getattr(pt, name).reshape(sh)
        x = getattr(got, name)
        chi, speed = SED[name]
        if speed not in w:
            assert _biteq(x, tend), name                                   # does not sediment in this configuration
            continue
        F = (cl["rho"] * cl[chi]) * w[speed]
        up = torch.cat([F[:, 1:], torch.zeros_like(F[:, :1])], dim=1)
        err = (x - (tend + (up - F) * g)).abs()
        tol = k_eps * (tend.abs() + (up + F) * g) + tiny
        assert bool((err <= tol).all()), (name, float((err - tol).max()))
        if name in ("dq_rai_dt", "dq_ice_dt"):
            pf = got.precip_rai if name == "dq_rai_dt" else got.precip_ice
            assert bool(((pf - F[:, 0]).abs() <= k_eps * F[:, 0]).all()), name


@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("limited", [True, False])
@pytest.mark.parametrize("cloud,vel", [(False, "sb"), (True, "chen")])
def test_step_equals_its_parts(dev, ft, limited, cloud, vel):
    d, dz, mp, tps = _case(dev, ft, 37, 20, seed=41, limited=limited)
    got = _step(d, dz, mp, tps, vel, cloud)
    torch.cuda.synchronize()
    _check_against_parts(got, d, dz, mp, tps, ft, limited, vel, cloud)
    assert bool(torch.isneginf(got.log_lambda).any()) and bool(torch.isfinite(got.log_lambda).any())
    assert float(got.precip_rai.max()) > 0 and float(got.precip_ice.max()) > 0


@pytest.fixture(scope="module")
def composed(dev, oracle):
    """One device call + one oracle composition per configuration, shared by the tests that need them (never modified)."""
    cache = {}

    def get(ft, limited, vel, cloud):
        key = (ft, limited, vel, cloud)
        if key not in cache:
            n_col, n_lev = 61, 24                                          # 1464 points: the oracle does about 8e3 P3 states per second
            d, dz, mp, tps = _case(dev, ft, n_col, n_lev, seed=7, limited=limited)
            shift = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (n_col, n_lev))).to(DT[ft]).to(dev)
            got = _step(d, dz, mp, tps, vel, cloud, inpc_log_shift=shift, brent_iters=40)
            torch.cuda.synchronize()
            ll = _np64(got.log_lambda)
            cols = {k: _np64(v) for k, v in d.items()}
            exp = R.expected(oracle, ft, cols, _np64(dz), np.where(np.isfinite(ll), ll, 0.0), limited=limited, vel=vel, cloud=cloud, shift=_np64(shift))
            cache[key] = (d, got, exp, cols)
        return cache[key]
    return get


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("limited,vel,cloud", [(True, "sb", True), (False, "chen", False)])
def test_against_the_oracle_composition(composed, oracle, ft, limited, vel, cloud):
    d, got, exp, cols = composed(ft, limited, vel, cloud)
    what = f"{ft} limited={limited} vel={vel} cloud={cloud}"
    # the states exercise what they claim
    ll = _np64(got.log_lambda)
    n_ice, n_none = R.check_log_lambda(oracle, ft, ll, cols, what=what)
    assert n_ice > 100 and n_none > 100
    if ft == "f32":
        rimed = (cols["b_rim"] * cols["rho"] > 42 * np.finfo(np.float32).eps) & (cols["q_rim"] > 0)        # B_rim above the blending band
        assert rimed.sum() > 100
    # all eight tendencies, every point; the ice speeds; the surface fluxes
    R.assert_tendencies({k: _np64(getattr(got, k)) for k in NAMES}, exp, ft, what=what)
    R.assert_ice_speeds(_np64(got.v_ice_n), _np64(got.v_ice_m), exp, ft, what=what)
    for k in ("precip_rai", "precip_ice"):
        x = _np64(getattr(got, k))
        np.testing.assert_allclose(x, exp[k], rtol=parity.RTOL[ft], atol=parity.FLOOR[ft])
        assert x.max() > 0, k


@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 1), (1, 2), (5, 3), (7, 5), (7, 74), (1, 600), (65, 9)])
def test_smallest_shapes_and_misaligned_twins(dev, ft, shape):
    """Levels shorter than a lane vector, columns that straddle a workgroup tile (255 vectors), a single column longer than a tile: each as in
    test_step_equals_its_parts, and bit for bit the same on misaligned twins of the buffers — every column shifted by one element (scalar head,
    vector body, scalar tail), and columns at different offsets modulo 16 B (one point per lane throughout)."""
    import cmx
    n_col, n_lev = shape
    n = n_col * n_lev
    d, dz, mp, tps = _case(dev, ft, n_col, n_lev, seed=31 + n_col + n_lev)
    got = _step(d, dz, mp, tps, "sb", True)
    torch.cuda.synchronize()
    _check_against_parts(got, d, dz, mp, tps, ft, True, "sb", True)
    for offs in ([1] * 24, [(3 * j + 1) % 4 for j in range(24)]):
        bufs = [torch.empty(n + 4, dtype=DT[ft], device=dev) for _ in range(22)]
        ins = {k: b[o:o + n].view(n_col, n_lev) for k, b, o in zip(R.IN_NAMES, bufs[:11], offs[:11])}
        for k in R.IN_NAMES:
            ins[k].copy_(d[k])
        pbuf = [torch.empty(n_col + 4, dtype=DT[ft], device=dev) for _ in range(2)]
        out = cmx.ColumnTendencies2MP3(*[b[o:o + n].view(n_col, n_lev) for b, o in zip(bufs[11:], offs[11:22])],
                                       *[b[o:o + n_col] for b, o in zip(pbuf, offs[22:])])
        cmx.column_tendencies_sedimentation_2m_p3(mp, tps, dz, *[ins[k] for k in R.IN_NAMES], vel=cmx.SB2006VelType, cloud_vel=P.StokesRegimeVelType(ft), out=out)
        torch.cuda.synchronize()
        for k in FIELDS:
            assert _biteq(getattr(out, k), getattr(got, k)), (k, offs[:4])


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_warm_start(composed, oracle, dev, ft):
    """A second call that starts from the first call's log λ lands on the same roots (the solver bound of tests/test_p3_gpu.py) and its tendencies
    meet the parity metric against the oracle composition at ITS log λ; no guess and a guess column of NaN are the same call bit for bit (the
    reference ignores a non-finite guess)."""
    import cmx
    limited, vel, cloud = True, "sb", True
    d, first, _, cols = composed(ft, limited, vel, cloud)
    n_col, n_lev = d["rho"].shape
    _, dz, mp, tps = _case(dev, ft, n_col, n_lev, seed=7, limited=limited)
    shift = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (n_col, n_lev))).to(DT[ft]).to(dev)
    second = _step(d, dz, mp, tps, vel, cloud, inpc_log_shift=shift, brent_iters=40, log_lambda_guess=first.log_lambda)
    torch.cuda.synchronize()
    a, b = _np64(first.log_lambda), _np64(second.log_lambda)
    assert np.array_equal(np.isneginf(a), np.isneginf(b))
    fin = np.isfinite(a)
    err = np.abs(b[fin] - a[fin]) / np.abs(a[fin])
    flipped = int((err > parity.RTOL[ft]).sum())
    print(f"\n[2M+P3 column] warm start {ft}: {int(fin.sum())} states with ice, {flipped} flipped, worst of the rest {err[err <= parity.RTOL[ft]].max():.3e}")
    assert flipped <= R.MAX_FLIPPED * fin.sum()
    exp = R.expected(oracle, ft, cols, _np64(dz), np.where(np.isfinite(b), b, 0.0), limited=limited, vel=vel, cloud=cloud, shift=_np64(shift))
    R.assert_tendencies({k: _np64(getattr(second, k)) for k in NAMES}, exp, ft, what=f"warm start {ft}")
    # NULL guess == NaN guess, at the reference's budget
    none = _step(d, dz, mp, tps, vel, cloud)
    nan = _step(d, dz, mp, tps, vel, cloud, log_lambda_guess=torch.full_like(d["rho"], float("nan")))
    torch.cuda.synchronize()
    for k in FIELDS:
        assert _biteq(getattr(none, k), getattr(nan, k)), k


def _nan_eq(a, b, mask):
    return _biteq(a[mask], b[mask])


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_nan_policy(dev, ft):
    """A NaN in a column of a species: every tendency of that point is NaN (the pointwise entry's rule), and in the cell BELOW the tendencies of
    the species that share its fall speeds — all four ice species, or the two rain moments — and nothing else anywhere."""
    n_col, n_lev, c, k = 9, 20, 4, 10
    d, dz, mp, tps = _case(dev, ft, n_col, n_lev, seed=77)
    for key in ("q_rai", "q_ice", "q_lcl"):                                # every species present at (c, k), so every flux there is live
        d[key][c, k] = {"q_rai": 1e-4, "q_ice": 2e-2, "q_lcl": 1e-4}[key]
    d["q_rim"][c, k], d["b_rim"][c, k] = 1e-2, 1e-2 / 300.0
    clean = _step(d, dz, mp, tps, "sb", True)
    mask = torch.ones(n_col, n_lev, dtype=torch.bool, device=dev)
    mask[c, k - 1:k + 1] = False
    ice, rain, cloud = NAMES[4:], NAMES[2:4], NAMES[:2]
    for col, hit, spared in (("q_ice", ice, rain + cloud), ("q_rai", rain, ice + cloud)):
        bad_in = dict(d)
        bad_in[col] = d[col].clone()
        bad_in[col][c, k] = float("nan")
        bad = _step(bad_in, dz, mp, tps, "sb", True)
        torch.cuda.synchronize()
        for name in NAMES:
            assert bool(torch.isnan(getattr(bad, name)[c, k])), (col, name)                # the point itself: all eight
        for name in hit:
            assert bool(torch.isnan(getattr(bad, name)[c, k - 1])), (col, name)            # receives the NaN flux from above
        for name in spared:
            assert _biteq(getattr(bad, name)[c, k - 1], getattr(clean, name)[c, k - 1]), (col, name)
        for name in NAMES:
            assert _nan_eq(getattr(bad, name), getattr(clean, name), mask), (col, name)
        for name in ("log_lambda", "v_ice_n", "v_ice_m"):
            keep = mask.clone()
            keep[c, k - 1] = True                                          # these are pointwise: only (c, k) may differ
            assert _nan_eq(getattr(bad, name), getattr(clean, name), keep), (col, name)
        assert _biteq(bad.precip_rai, clean.precip_rai) and _biteq(bad.precip_ice, clean.precip_ice)      # level 10 is not the surface


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_graph_capture(dev, ft):
    """The entry is a pure sequence of launches on the caller's stream: captured on a side stream and replayed once, it writes what the eager call
    writes, bit for bit."""
    import cmx
    n_col, n_lev = 37, 20
    d, dz, mp, tps = _case(dev, ft, n_col, n_lev, seed=5)
    guess = torch.full_like(d["rho"], 9.0)
    kw = dict(vel=cmx.Chen2022VelTypeRain, cloud_vel=P.StokesRegimeVelType(ft), log_lambda_guess=guess)
    cols = [d[k] for k in R.IN_NAMES]
    eager = cmx.column_tendencies_sedimentation_2m_p3(mp, tps, dz, *cols, want_precip_flux=True, **kw)
    out = cmx.ColumnTendencies2MP3(*[torch.full_like(d["rho"], float("nan")) for _ in range(11)],
                                   *[torch.full((n_col,), float("nan"), dtype=DT[ft], device=dev) for _ in range(2)])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cmx.column_tendencies_sedimentation_2m_p3(mp, tps, dz, *cols, out=out, **kw)
    torch.cuda.synchronize()
    for t in out:
        t.fill_(float("nan"))                                              # whatever capture left behind: the replay must write every value
    graph.replay()
    torch.cuda.synchronize()
    for k in FIELDS:
        assert _biteq(getattr(out, k), getattr(eager, k)), k
