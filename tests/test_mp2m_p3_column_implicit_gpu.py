"""The 2M + P3 column step with backward-Euler sedimentation on the device (cmx_mp2m_p3_column_implicit_sedimentation_*, cmx.column_implicit_sedimentation_2m_p3;
include/cmx.h §24):

    G_k = top ? B_k : fma(A_k, G_{k+1}, B_k),     out_k = fma(top ? 0 : G_{k+1}, g, fma(−F_k, g, a_k))·r_k,     surface outputs G_0 of q_rai and q_ice

— dt = 0 and inv_dz = 0 against the explicit entry (9b) as values, the defining identity against it, the surface relation and the column budget, the lower bound
"no negativity of its own" at Courant numbers of up to a hundred (where the explicit entry falls below it), independence of the other columns and of alignment,
the NaN rule, graph capture and `out=`.  Both float types, (cloud, vel) ∈ {(False, sb), (True, chen)}, the states of tests/p3_column_ref.py; no call has
more than 4 200 points.  The Float64 recipe and the bounds, with their derivations: tests/p3_column_implicit_cases.py (self-checked in
tests/test_mp2m_p3_column_implicit_host.py)."""
import numpy as np
import pytest
import torch

import p3_column_implicit_cases as PC
import p3_column_ref as R
from test_column_implicit_average_gpu import _eq      # same values, NaN = NaN, −0 = +0
import cmx
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}
FTS = ["f64", "f32"]
CONFIGS = [(False, "sb"), (True, "chen")]
NAMES = R.NAMES
POINTWISE = ("log_lambda", "v_ice_n", "v_ice_m")
FIELDS = NAMES + POINTWISE + ("precip_rai", "precip_ice")
# species → (state column, fall speed); the cloud pair falls only with cloud_vel
SED = {"dq_lcl_dt": ("q_lcl", "c_m"), "dn_lcl_dt": ("n_lcl", "c_n"), "dq_rai_dt": ("q_rai", "w_m"), "dn_rai_dt": ("n_rai", "w_n"),
       "dq_ice_dt": ("q_ice", "v_m"), "dn_ice_dt": ("n_ice", "v_n"), "dq_rim_dt": ("q_rim", "v_m"), "db_rim_dt": ("b_rim", "v_m")}
PRECIP = {"dq_rai_dt": "precip_rai", "dq_ice_dt": "precip_ice"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _biteq(a, b):
    """Equal bit for bit (−Inf, NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def _vel(name):
    return cmx.SB2006VelType if name == "sb" else cmx.Chen2022VelTypeRain


def _case(dev, ft, shape, nonneg=False, limited=True):
    """(state columns, inv_dz, mp, tps) of the shape; `nonneg`: ρ and the species clamped at 0 (the lower bound is stated for χ = χ⁺); `limited`: the rain PSD
    variant of the parameters, as in tests/test_mp2m_p3_column_gpu.py."""
    n_col, n_lev = shape
    s = R.states(n_col, n_lev, seed=31 + n_col + n_lev, f32_safe=(ft == "f32"))
    d = {k: torch.from_numpy(v).to(DT[ft]).to(dev) for k, v in s.items()}
    if nonneg:
        d = {k: (v if k in ("T", "q_tot") else v.clamp(min=0)) for k, v in d.items()}
    dz = torch.from_numpy(R.inv_dz(n_lev, seed=n_lev)).to(DT[ft]).to(dev)
    return d, dz, P.Microphysics2MParams(ft, with_ice=True, is_limited=limited), P.ThermodynamicsParameters(ft)


def _kw(ft, vel, cloud):
    return dict(vel=_vel(vel), cloud_vel=P.StokesRegimeVelType(ft) if cloud else None)


def _explicit(d, dz, mp, tps, ft, vel, cloud, **kw):
    return cmx.column_tendencies_sedimentation_2m_p3(mp, tps, dz, *[d[k] for k in R.IN_NAMES], want_precip_flux=True, **_kw(ft, vel, cloud), **kw)


def _implicit(d, dz, mp, tps, ft, vel, cloud, dt, **kw):
    kw.setdefault("want_precip_flux", True)
    return cmx.column_implicit_sedimentation_2m_p3(mp, tps, dz, *[d[k] for k in R.IN_NAMES], dt, **_kw(ft, vel, cloud), **kw)


def _np(t):
    return t.double().cpu().numpy()


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("limited", [True, False])
@pytest.mark.parametrize("cloud,vel", CONFIGS)
def test_without_a_step_the_entry_is_the_explicit_entry(dev, ft, cloud, vel, limited):
    """dt = 0 on every shape around the kernel's chunk of 256 points: c = 0, r = 1, A = 0, G = F — the eight tendencies and the two surface fluxes are the (9b)
    entry's as values (a −0 may become +0 at a column top).  log λ and the ice fall speeds are that entry's bits at every dt: the same launches.  With the
    limited and with the not-limited rain PSD: both halves of the kernel's instantiations."""
    moved = 0
    for shape in PC.SHAPES:
        d, dz, mp, tps = _case(dev, ft, shape, limited=limited)
        want = _explicit(d, dz, mp, tps, ft, vel, cloud)
        got = _implicit(d, dz, mp, tps, ft, vel, cloud, 0.0)
        for k in NAMES + ("precip_rai", "precip_ice"):
            x, y = getattr(got, k), getattr(want, k)
            assert bool(torch.isfinite(y).all()) and _eq(x, y), (shape, k, int((x != y).sum()))
        for dt in (0.0,) + PC.DTS:
            other = got if dt == 0.0 else _implicit(d, dz, mp, tps, ft, vel, cloud, dt)
            for k in POINTWISE:
                assert _biteq(getattr(other, k), getattr(want, k)), (shape, dt, k)
            if dt == 300.0:
                moved += int((other.dq_ice_dt != want.dq_ice_dt).sum())
        assert got.precip_rai.shape == (shape[0],)
    assert moved > 1000      # … and at dt = 300 the step is not the explicit one


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("cloud,vel", CONFIGS)
def test_without_levels_the_step_is_the_pointwise_tendencies(dev, ft, cloud, vel):
    """inv_dz ≡ 0: c = 0, r = 1, g = 0 — for every Δt the eight tendencies are the (9b) entry's with the same zero inv_dz (which are the pointwise entry's)."""
    for shape in ((37, 20), (65, 63), (2, 600)):
        d, dz, mp, tps = _case(dev, ft, shape)
        zero = torch.zeros_like(dz)
        want = _explicit(d, zero, mp, tps, ft, vel, cloud)
        for dt in PC.DTS:
            got = _implicit(d, zero, mp, tps, ft, vel, cloud, dt)
            for k in NAMES:
                x, y = getattr(got, k), getattr(want, k)
                assert bool(torch.isfinite(y).all()) and _eq(x, y), (shape, dt, k, int((x != y).sum()))
            for k in POINTWISE:
                assert _biteq(getattr(got, k), getattr(want, k)), (shape, dt, k)


def _terms(dev, ft, shape, cloud, vel, dt, nonneg=False):
    """Everything the host-side properties need, as Float64 arrays over the FALLING species [6 or 8, n_col, n_lev]: out and G_0 of the implicit entry, out_expl
    and F_0 of the (9b) entry, a (the (9b) entry at zero inv_dz), the fall speeds — rain: the warm-rain tendencies entry; cloud: cmx.cloud_terminal_velocity; ice:
    the call's own outputs —, χ⁺, ρ, inv_dz."""
    d, dz, mp, tps = _case(dev, ft, shape, nonneg)
    impl = _implicit(d, dz, mp, tps, ft, vel, cloud, dt)
    expl = _explicit(d, dz, mp, tps, ft, vel, cloud)
    pt = _explicit(d, torch.zeros_like(dz), mp, tps, ft, vel, cloud)
    flat = {k: v.reshape(-1) for k, v in d.items()}
    warm = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), P.Microphysics2MParams(ft), tps, *[flat[k] for k in R.IN_NAMES[:7]], vel=_vel(vel))
    cl = {k: v.clamp(min=0) for k, v in d.items()}
    w = {"w_n": warm.vt_rai_n.reshape(shape), "w_m": warm.vt_rai_m.reshape(shape), "v_n": impl.v_ice_n, "v_m": impl.v_ice_m}
    if cloud:
        cv = cmx.cloud_terminal_velocity(mp.warm_rain.c.seifert_beheng.pdf_c, P.StokesRegimeVelType(ft), cl["q_lcl"].reshape(-1), cl["rho"].reshape(-1),
                                         (cl["rho"] * cl["n_lcl"]).reshape(-1))
        w["c_n"], w["c_m"] = cv.vt_n.reshape(shape), cv.vt_m.reshape(shape)
    torch.cuda.synchronize()
    names = [n for n in NAMES if SED[n][1] in w]
    assert len(names) == (8 if cloud else 6)
    stack = lambda r: np.stack([_np(getattr(r, n)) for n in names])  # noqa: E731
    t = dict(names=names, out=stack(impl), expl=stack(expl), a=stack(pt), w=np.stack([_np(w[SED[n][1]]) for n in names]),
             chi=np.stack([_np(cl[SED[n][0]]) for n in names]), rho=_np(cl["rho"]), inv_dz=_np(dz),
             G0={n: _np(getattr(impl, PRECIP[n])) for n in PRECIP}, F0={n: _np(getattr(expl, PRECIP[n])) for n in PRECIP})
    for k in ("out", "expl", "a", "w"):
        assert np.isfinite(t[k]).all(), k
    t["F"] = t["rho"][None] * t["chi"] * t["w"]
    idz = t["inv_dz"][None, None, :]
    t["c"], t["beta"], t["g"] = dt * t["w"] * idz, dt * t["w"] * t["rho"][None], idz / t["rho"][None]
    return t


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("cloud,vel", CONFIGS)
def test_the_defining_identity_the_surface_relation_and_the_budget(dev, ft, cloud, vel):
    """In Float64 on the host, for every falling species and every element:  out_k (1 + c_k) − out_expl_k = g_k β_{k+1} out_{k+1}  (top: right side 0) with
    out_expl the (9b) entry on the same inputs — with the top condition this triangular set pins every output —, within M_IDENTITY·eps(FT)·S.  The surface
    relation G_0 = F_0 + β_0 out_0 (F_0: the (9b) entry's surface flux) and the column budget Σ_k ρ_k out_k Δz_k + G_0 = Σ_k ρ_k a_k Δz_k (within
    M_BUDGET·eps(FT)·scale) are asserted for q_rai and q_ice ONLY, not for all falling species: both need G_0, and the entry hands out G_0 of these two
    (`precip_rai`, `precip_ice`) and of no other species.  The outputs of the other species are pinned by the identity alone.  The multiples and the scales —
    the surface and budget scales hold one term more than those of column_implicit_step_cases, because the tendency is not limited — are derived in
    tests/p3_column_implicit_cases.py."""
    eps = PC.EPS[ft]
    for shape in ((37, 20), (2, 600)):
        for dt in PC.DTS:
            t = _terms(dev, ft, shape, cloud, vel, dt)
            res, S = PC.identity(t["out"], t["expl"], t["a"], t["F"], t["c"], t["beta"], t["g"])
            worst = float((res / np.maximum(S, 1e-300)).max() / eps)
            sworst = bworst = 0.0
            checks = []
            for n, j in ((n, t["names"].index(n)) for n in PRECIP):
                sres, ssc = PC.surface(t["G0"][n], t["F0"][n], t["beta"][j, :, 0], t["out"][j, :, 0], t["c"][j, :, 0], t["a"][j, :, 0])
                bres, bsc = PC.budget(t["out"][j:j + 1], t["G0"][n][None], t["a"][j:j + 1], t["rho"], t["inv_dz"])
                sworst = max(sworst, float((sres / np.maximum(ssc, 1e-300)).max() / eps))
                bworst = max(bworst, float((bres / np.maximum(bsc, 1e-300)).max() / eps))
                checks.append((n, bool((sres <= PC.M_IDENTITY * eps * ssc).all()), bool((bres <= PC.M_BUDGET * eps * bsc).all())))
                assert np.abs(t["G0"][n]).max() > 0, n      # (G_0 < 0 happens: a sink larger than the content, unlimited, leaves a deficit that falls)
            print(f"{ft} cloud={cloud} {vel} {shape} dt={dt:g}: c max {t['c'].max():.3g}; identity {worst:.3g} eps S (M {PC.M_IDENTITY:g}), "
                  f"surface {sworst:.3g} eps (M {PC.M_IDENTITY:g}), budget {bworst:.3g} eps (M {PC.M_BUDGET:g})")
            assert bool((res <= PC.M_IDENTITY * eps * S).all()), (shape, dt, worst)
            assert all(s and b for _, s, b in checks), (shape, dt, checks, sworst, bworst)
            if dt == 300.0:
                assert t["c"].max() > 20.0 and (np.abs(t["out"] - t["a"]) > 0).mean() > 0.25      # sedimentation moved a good share of the elements


# the share of the falling cells where the (9b) entry's result lies below the same lower bound at Δt = 300: the oracle's tendencies and fall speeds give 32–38 %
# on these states; the floor asserted is the issue's
EXPLICIT_BELOW_FLOOR = 0.10


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("cloud,vel", CONFIGS)
def test_the_step_adds_no_negativity_of_its_own(dev, ft, cloud, vel):
    """Non-negative states, every element of every falling species: χ_k + Δt out_k ≥ r_k (p⁻_k + Δt g_k G⁻_{k+1}) − m·eps(FT)·scale with p = χ + Δt a,
    p⁻ = min(p, 0) and G⁻ the Float64 recurrence on B⁻ = w ρ⁺ r p⁻ — what the tendencies alone and the deficits falling in from above account for (the tendency
    of §24 is not limited); scale: `positivity`'s, m: p3_column_implicit_cases.m_lower.  The Float64 recipe itself stays within 2.3 eps·scale of the bound on
    (37, 20).  At Δt = 300 the (9b) entry's result on the same states lies below the same bound in a good share of the falling cells."""
    eps = PC.EPS[ft]
    cells = below = 0
    for shape in ((37, 20), (65, 63), (2, 600)):
        for dt in PC.DTS:
            t = _terms(dev, ft, shape, cloud, vel, dt, nonneg=True)
            margin, sc, m = PC.lower_bound_margin(t["chi"], t["out"], t["a"], t["F"], t["w"], t["rho"], t["inv_dz"], dt)
            worst1 = float((-margin / np.maximum(sc, 1e-300)).max() / eps)
            worst = float((-margin / np.maximum(sc, 1e-300) / m).max() / eps)
            host = PC.recipe(t["a"], t["F"], t["w"], t["rho"], t["inv_dz"], dt)[0]
            hm = PC.lower_bound_margin(t["chi"], host, t["a"], t["F"], t["w"], t["rho"], t["inv_dz"], dt)[0]
            hworst = float((-hm / np.maximum(sc, 1e-300)).max() / PC.EPS["f64"])
            falling = t["w"] > 0
            em = PC.lower_bound_margin(t["chi"], t["expl"], t["a"], t["F"], t["w"], t["rho"], t["inv_dz"], dt)[0]
            low = falling & (em < -m * eps * sc)
            print(f"{ft} cloud={cloud} {vel} {shape} dt={dt:g}: c max {t['c'].max():.3g}, cells with c > 1: {float((t['c'] > 1).mean()):.2f}; worst shortfall "
                  f"{worst1:.3g} eps·scale, {worst:.3g} of m; host recipe {hworst:.3g} eps(f64)·scale; p < 0 in {float((t['chi'] + dt * t['a'] < 0).mean()):.2f}; "
                  f"explicit below the bound: {int(low.sum())} of {int(falling.sum())} falling cells")
            assert bool((margin >= -m * eps * sc).all()), (shape, dt, worst1, worst)
            if shape == (37, 20):
                assert hworst <= 2.3, (dt, hworst)
            if dt == 300.0:
                cells += int(falling.sum())
                below += int(low.sum())
    print(f"{ft} cloud={cloud} {vel}: at dt = 300 the explicit entry lies below the bound in {below} of {cells} falling cells")
    assert cells > 3000 and below >= EXPLICIT_BELOW_FLOOR * cells, (below, cells)


def _shifted(t):
    """The same values in storage that starts one element into its buffer."""
    return torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:].view(t.shape)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("limited", [True, False])
@pytest.mark.parametrize("cloud,vel", CONFIGS)
def test_results_do_not_depend_on_the_other_columns_or_on_alignment(dev, ft, cloud, vel, limited):
    """Columns [0:3] of (65, 63) run alone equal the slice of the full call bit for bit — a workgroup owns 16 columns of the full call, chunk edges at 256, 512
    and 768 points, while the three alone make one chunk —, and so do both calls on misaligned twins: every column, inv_dz and every output shifted by one
    element (the pointwise launches take their scalar head / vector body / scalar tail path, the new kernel any address)."""
    shape, dt = (65, 63), 300.0
    d, dz, mp, tps = _case(dev, ft, shape, limited=limited)
    full = _implicit(d, dz, mp, tps, ft, vel, cloud, dt)
    assert all(bool(torch.isfinite(getattr(full, k)).all()) for k in NAMES)
    head = {k: v[:3].contiguous() for k, v in d.items()}
    alone = _implicit(head, dz, mp, tps, ft, vel, cloud, dt)
    for k in FIELDS:
        assert _biteq(getattr(alone, k), getattr(full, k)[:3]), k
    for cols, ref in ((d, full), (head, alone)):
        n_col = cols["rho"].shape[0]
        n = n_col * shape[1]
        twins = {k: _shifted(v) for k, v in cols.items()}
        bufs = [torch.full((n + 2,), -7.0, dtype=DT[ft], device=dev) for _ in range(11)]
        pbufs = [torch.full((n_col + 2,), -7.0, dtype=DT[ft], device=dev) for _ in range(2)]
        out = cmx.ColumnTendencies2MP3(*[b[1:-1].view(n_col, shape[1]) for b in bufs], *[b[1:-1] for b in pbufs])
        assert all(t.data_ptr() % 16 != 0 for t in list(twins.values()) + list(out))
        got = _implicit(twins, _shifted(dz), mp, tps, ft, vel, cloud, dt, out=out)
        torch.cuda.synchronize()
        for k in FIELDS:
            assert _biteq(getattr(got, k), getattr(ref, k)), (n_col, k)
        assert all(float(b[0]) == float(b[-1]) == -7.0 for b in bufs + pbufs)      # nothing written outside the columns


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("cloud,vel", CONFIGS)
def test_the_nan_rule(dev, ft, cloud, vel):
    """A NaN in q_ice at (col, l) of (4, 64): every tendency of the point is NaN (the pointwise rule), so B of every falling species is, and the recurrence carries
    it down — every falling species is non-finite at the levels ≤ l of that column, and so are the column's surface fluxes; the levels > l and the other columns
    keep their bits; without cloud_vel the two cloud columns do not fall: below l they are finite and keep their bits."""
    shape, col, lev, dt = (4, 64), 2, 40, 300.0
    d, dz, mp, tps = _case(dev, ft, shape)
    clean = _implicit(d, dz, mp, tps, ft, vel, cloud, dt)
    assert all(bool(torch.isfinite(getattr(clean, k)).all()) for k in NAMES)
    bad_in = dict(d)
    bad_in["q_ice"] = d["q_ice"].clone()
    bad_in["q_ice"][col, lev] = float("nan")
    bad = _implicit(bad_in, dz, mp, tps, ft, vel, cloud, dt)
    torch.cuda.synchronize()
    hit = torch.zeros(shape, dtype=torch.bool, device=dev)
    hit[col, :lev + 1] = True
    other = torch.arange(shape[0], device=dev) != col
    for k in NAMES:
        x, y = getattr(bad, k), getattr(clean, k)
        assert _biteq(x[other], y[other]), k                                   # the other columns
        assert _biteq(x[col, lev + 1:], y[col, lev + 1:]), k                   # the levels above
        assert not bool(torch.isfinite(x[col, lev]).any()), k                  # the point itself: all eight
        if cloud or k not in ("dq_lcl_dt", "dn_lcl_dt"):
            assert not bool(torch.isfinite(x[hit]).any()), k
        else:
            assert bool(torch.isfinite(x[col, :lev]).all()) and _biteq(x[col, :lev], y[col, :lev]), k
    for k in ("precip_rai", "precip_ice"):
        x, y = getattr(bad, k), getattr(clean, k)
        assert not bool(torch.isfinite(x[col])) and _biteq(x[other], y[other]), k
    keep = torch.ones(shape, dtype=torch.bool, device=dev)
    keep[col, lev] = False
    for k in POINTWISE:                                                        # pointwise: only (col, l) may differ
        assert _biteq(getattr(bad, k)[keep], getattr(clean, k)[keep]), k


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("cloud,vel", CONFIGS)
def test_graph_capture_and_out(dev, ft, cloud, vel):
    """The entry is a pure sequence of launches on the caller's stream: captured on a side stream and replayed once, it writes what the eager call writes, bit for
    bit; `out=` is used as given, the surface-flux vectors included."""
    shape, dt = (37, 20), 300.0
    d, dz, mp, tps = _case(dev, ft, shape)
    guess = torch.full_like(d["rho"], 9.0)
    eager = _implicit(d, dz, mp, tps, ft, vel, cloud, dt, log_lambda_guess=guess)
    out = cmx.ColumnTendencies2MP3(*[torch.full_like(d["rho"], float("nan")) for _ in range(11)],
                                   *[torch.full((shape[0],), float("nan"), dtype=DT[ft], device=dev) for _ in range(2)])
    got = _implicit(d, dz, mp, tps, ft, vel, cloud, dt, log_lambda_guess=guess, out=out)
    torch.cuda.synchronize()
    assert got is out
    for k in FIELDS:
        assert _biteq(getattr(out, k), getattr(eager, k)), k
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _implicit(d, dz, mp, tps, ft, vel, cloud, dt, log_lambda_guess=guess, out=out)
    torch.cuda.synchronize()
    for t in out:
        t.fill_(float("nan"))                                                  # whatever capture left behind: the replay must write every value
    graph.replay()
    torch.cuda.synchronize()
    for k in FIELDS:
        assert _biteq(getattr(out, k), getattr(eager, k)), k
    # without want_precip_flux and without out= there are no surface vectors
    none = _implicit(d, dz, mp, tps, ft, vel, cloud, dt, log_lambda_guess=guess, want_precip_flux=False)
    assert none.precip_rai is None and none.precip_ice is None and _biteq(none.dq_ice_dt, eager.dq_ice_dt)
