"""The column steps with the sub-stepped implicit average as tendency operator on the device (cmx_sb2006_column_implicit_average_sedimentation_*,
cmx_mp1m_column_implicit_average_sedimentation_*; cmx.column_implicit_average_sedimentation_2m / _1m; include/cmx.h §20):

    out_j = fma(top ? 0 : F_j[k+1], g, fma(−F_j[k], g, a_j))

with a_j the average entry's result (§19) in every bit, F the existing column entry's fluxes in every bit, the sedimentation term the existing column
entry's to rounding; independence of the kernel's tiles, the NaN rule, alignment, the wrappers' checks, graph capture and `out=`.

Both schemes, both float types, the option cases of implicit_average_cases.CASES; the shapes sit around the kernel's tile (a 256-lane workgroup owns 255 points and
reads the 256th) and the column top: one point, columns that end exactly at a tile edge, columns that straddle one, n_lev = 1 (every point a top), a tail tile.  No call has more than 4 200 points."""
import ctypes as C

import numpy as np
import pytest
import torch

import implicit_average_cases as AC
import jacobian_products_cases as PC
import cmx
from cmx import _abi, _lib
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
EPS = {"f32": 2.0 ** -23, "f64": 2.0 ** -52}
FTS = ["f64", "f32"]
SHAPES = [(1, 1), (1, 255), (1, 257), (3, 85), (4, 64), (65, 63), (7, 1), (2, 2)]
BIG = (65, 63)
# the flux options: SB2006 (rain velocity scheme, cloud sedimentation) — "steep" is the Chen-2022 table the Γ fit cannot represent (run-time Γ);
# 1-moment: the default Chen-2022 rain table and the run-time-Γ one
FLUX = {"sb2006": [("sb", False), ("sb", True), ("chen", False), ("chen", True), ("steep", True)], "mp1m": ["default", "steep"]}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _eq(a, b):
    """Same bits, NaN = NaN (−0 = +0)."""
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


def _inv_dz(n_lev, ft, dev, zero=False):
    g = torch.Generator().manual_seed(n_lev)
    dz = 1.0 / (30.0 + 470.0 * torch.rand(n_lev, generator=g, dtype=torch.float64))
    return (dz * (0.0 if zero else 1.0)).to(DT[ft]).to(dev)


def _host_state(oracle, name, shape):
    """The scheme's state set of tests/implicit_cases.py, thinned evenly to the shape (every subset and the pinned last point are represented), as Float64."""
    full = AC.STATES[name](oracle)
    n = shape[0] * shape[1]
    idx = np.linspace(0, full[0].size - 1, n).round().astype(np.int64)
    return [np.array(c[idx], dtype=np.float64) for c in full]


def _state(oracle, name, shape, ft, dev):
    return [torch.from_numpy(c).to(DT[ft]).reshape(shape).to(dev) for c in _host_state(oracle, name, shape)]


class Step:
    """One scheme, option case, float type and flux option: the fused step, the existing column step, the average entry and the tendencies entry."""

    def __init__(self, name, case, ft, flux):
        self.name, self.ft, self.flux = name, ft, flux
        self.mp = PC.SCHEMES[name].params(ft, case)
        self.tps = P.ThermodynamicsParameters(ft)
        if name == "sb2006":
            vel, cloud = flux
            self.vel = cmx.SB2006VelType if vel == "sb" else cmx.Chen2022VelTypeRain
            self.velp = P.rain_vel_params(ft)
            if vel == "steep":
                self.velp.chen2022.b_rho = 0.6
            self.cloud = P.StokesRegimeVelType(ft) if cloud else None
        else:
            self.vels = (P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft), P.Chen2022VelTypeIce(ft))
            if flux == "steep":
                self.vels[1].b_rho = 0.6

    def fused(self, inv_dz, cols, dt, nsub, nonneg=True, **kw):
        """([4, n_col, n_lev] outputs, the surface fluxes)"""
        if self.name == "sb2006":
            r = cmx.column_implicit_average_sedimentation_2m(self.mp, self.tps, inv_dz, *cols, dt, nsub, nonneg, vel=self.vel, vel_params=self.velp,
                                                             cloud_vel=self.cloud, want_precip_flux=True, **kw)
            return torch.stack(list(r[:4])), [r.precip_flux]
        r = cmx.column_implicit_average_sedimentation_1m(self.mp, self.tps, *self.vels, inv_dz, *cols, dt, nsub, nonneg, **kw)
        return torch.stack(list(r[:4])), [r.precip_rai, r.precip_sno]

    def column(self, inv_dz, cols):
        """The existing column entry, instantaneous tendencies."""
        if self.name == "sb2006":
            r = cmx.column_tendencies_sedimentation(self.mp, self.tps, inv_dz, *cols, vel=self.vel, vel_params=self.velp, cloud_vel=self.cloud,
                                                    want_precip_flux=True)
            return torch.stack(list(r[:4])), [r.precip_flux]
        r = cmx.column_tendencies_sedimentation_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), self.mp, self.tps, *self.vels, inv_dz, *cols)
        return torch.stack(list(r[:4])), [r.precip_rai, r.precip_sno]

    def average(self, cols, dt, nsub, nonneg=True):
        """The average entry (§19) on the flattened states, [4, n_col, n_lev]."""
        flat = [c.reshape(-1) for c in cols]
        fn = cmx.warm_rain_implicit_average_2m if self.name == "sb2006" else cmx.implicit_average_1m
        return fn(self.mp, self.tps, *flat, dt, nsub, nonneg).reshape(4, *cols[0].shape)

    def tendencies(self, cols):
        flat = [c.reshape(-1) for c in cols]
        if self.name == "sb2006":
            r = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), self.mp, self.tps, *flat)
        else:
            r = cmx.bulk_microphysics_tendencies_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), self.mp, self.tps, *flat)
        return torch.stack(list(r[:4])).reshape(4, *cols[0].shape)


def _assert_regular(cols):
    """The precondition of the g = 0 comparison, on the INPUTS: finite states with 0 < ρ ≤ 2 kg/m³ (the range of the fitted Chen-2022 Γ), so that every
    flux is finite and g = 0·(1/ρ) = 0."""
    for c in cols:
        assert bool(torch.isfinite(c).all())
    assert bool((cols[0] > 0).all()) and bool((cols[0] <= 2.0).all())


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_the_tendency_part_is_the_average_entry_in_every_bit(dev, oracle, name, case, ft):
    """inv_dz ≡ 0: both fma terms vanish and the four outputs are the average entry's on the flattened states — nsub ∈ {1, 2, 5}, Δt ∈ {1, 30, 300}, limiter on
    and off, every shape; the flux options rotate over the shapes.  The fluxes are finite here (and the existing column entry says so too)."""
    for k, shape in enumerate(SHAPES):
        step = Step(name, case, ft, FLUX[name][k % len(FLUX[name])])
        cols = _state(oracle, name, shape, ft, dev)
        _assert_regular(cols)
        zero = _inv_dz(shape[1], ft, dev, zero=True)
        assert all(bool(torch.isfinite(p).all()) for p in step.column(zero, cols)[1])
        for dt in AC.DTS:
            for nsub in AC.NSUBS:
                for nonneg in (True, False):
                    got, _ = step.fused(zero, cols, dt, nsub, nonneg)
                    want = step.average(cols, dt, nsub, nonneg)
                    assert _eq(got, want), (shape, step.flux, dt, nsub, nonneg, int(((got != want) & ~(torch.isnan(got) & torch.isnan(want))).sum()))


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_the_surface_fluxes_are_the_existing_column_entry_s_in_every_bit(dev, oracle, name, case, ft):
    """precip_flux; precip_rai, precip_sno against the existing column entry in instantaneous mode, same states and options: both rain velocity schemes and
    the run-time-Γ table, with and without cloud_vel; 1-moment default and run-time-Γ parameters."""
    nonzero = 0
    for shape in SHAPES:
        cols = _state(oracle, name, shape, ft, dev)
        inv_dz = _inv_dz(shape[1], ft, dev)
        for flux in FLUX[name]:
            step = Step(name, case, ft, flux)
            got, want = step.fused(inv_dz, cols, 30.0, 1)[1], step.column(inv_dz, cols)[1]
            for g, w in zip(got, want):
                assert g.shape == (shape[0],) and _eq(g, w), (shape, flux)
                nonzero += int((w > 0).sum())
    assert nonzero > 100      # the comparison is not one of zeros


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_the_sedimentation_term_is_the_existing_column_entry_s(dev, oracle, name, case, ft):
    """In Float64 on the host, per element: (out − a) against (col_inst − tend_inst) within 4·eps(FT)·(|a| + |tend_inst| + |F g| + |F_up g|) — each side is two
    fused roundings of quantities bounded by that sum (≤ 3 eps·sum in all), one eps for the host subtraction.  The two flux magnitudes come from a Float64
    DEVICE run of the existing column entry: with n_lev = 1 and inv_dz = 1 every point is a top and tend − col = F/ρ⁺ (to a Float64 rounding of the
    tendency); then |F g|_k = |F/ρ|_k·inv_dz_k and |F_up g|_k = |F/ρ|_{k+1}·ρ_{k+1}/ρ_k·inv_dz_k.  No state is set aside."""
    total = moved = 0
    for k, shape in enumerate(SHAPES):
        flux = FLUX[name][k % len(FLUX[name])]
        step, step64 = Step(name, case, ft, flux), Step(name, case, "f64", flux)
        cols = _state(oracle, name, shape, ft, dev)
        inv_dz = _inv_dz(shape[1], ft, dev)
        assert bool((inv_dz > 0).all())
        out = step.fused(inv_dz, cols, 30.0, 2)[0].double().cpu().numpy()
        a = step.average(cols, 30.0, 2).double().cpu().numpy()
        col = step.column(inv_dz, cols)[0].double().cpu().numpy()
        tend = step.tendencies(cols).double().cpu().numpy()
        # the flux magnitudes, Float64 on the device from the same (FT) states
        c64 = [c.double().reshape(-1, 1) for c in cols]
        one = torch.ones(1, dtype=torch.float64, device=dev)
        phi = (step64.tendencies(c64) - step64.column(one, c64)[0]).abs().reshape(4, *shape).cpu().numpy()      # |F/ρ|
        rho = cols[0].double().cpu().numpy()
        dz = inv_dz.double().cpu().numpy()[None, :]
        Fg = phi * dz
        Fup = np.zeros_like(phi)
        Fup[:, :, :-1] = phi[:, :, 1:] * (rho[:, 1:] / rho[:, :-1]) * dz[:, :-1]
        bound = 4.0 * EPS[ft] * (np.abs(a) + np.abs(tend) + Fg + Fup)
        err = np.abs((out - a) - (col - tend))
        worst = float(np.nanmax(err / np.maximum(bound, 1e-300)))
        print(f"{name} {case} {ft} {shape} {flux}: max error / bound = {worst:.3g}")
        assert np.isfinite(out).all() and bool((err <= bound).all()), (shape, flux, worst)
        total += out.size
        moved += int((np.abs(out - a) > 0).sum())
    print(f"{name} {case} {ft}: sedimentation moved {moved} of {total} elements")
    assert moved >= total / 4, (moved, total)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_results_do_not_depend_on_the_tiles(dev, oracle, name, case, ft):
    """Each column run alone equals its row of the full call; the first m columns of a call equal the call on those columns; NaNs in the column that
    follows a column in memory leave every other column's bits alone — the top level has no inflow."""
    for k, shape in enumerate(SHAPES[3:6]):      # (3, 85), (4, 64), (65, 63): columns end inside, at and across the tile edges
        step = Step(name, case, ft, FLUX[name][(k + 1) % len(FLUX[name])])
        cols = _state(oracle, name, shape, ft, dev)
        inv_dz = _inv_dz(shape[1], ft, dev)
        full, precip = step.fused(inv_dz, cols, 30.0, 2)
        for c in sorted({0, 1, shape[0] // 2, shape[0] - 1}):
            alone, p = step.fused(inv_dz, [x[c:c + 1].contiguous() for x in cols], 30.0, 2)
            assert _eq(alone[:, 0], full[:, c]) and all(_eq(pa[0], pf[c]) for pa, pf in zip(p, precip)), (shape, c)
        for m in (1, 2, shape[0] - 1):
            head, p = step.fused(inv_dz, [x[:m].contiguous() for x in cols], 30.0, 2)
            assert _eq(head, full[:, :m]) and all(_eq(pa, pf[:m]) for pa, pf in zip(p, precip)), (shape, m)
        for c in (1, shape[0] - 1):
            bad = [x.clone() for x in cols]
            for x in bad:
                x[c] = float("nan")
            got, p = step.fused(inv_dz, bad, 30.0, 2)
            keep = torch.arange(shape[0], device=dev) != c
            assert bool(torch.isnan(got[:, c]).all()) and _eq(got[:, keep], full[:, keep]), (shape, c)
            assert all(_eq(pa[keep], pf[keep]) for pa, pf in zip(p, precip)), (shape, c)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_the_nan_rule(dev, oracle, name, case, ft):
    """A NaN in T at one point: that point's four outputs and nothing else.  A NaN in q_rai at level k: the point's outputs and the rain outputs of level
    k − 1 (SB2006: a NaN in a species poisons the point's fluxes, so every falling species of level k − 1); level k + 1, the rest of the column and the other
    columns keep their bits.  At a tile edge (flat index 255: the first point of the second workgroup, which the first one reads for its fluxes) and
    inside a tile."""
    shape = BIG
    step = Step(name, case, ft, FLUX[name][1])      # SB2006: with cloud sedimentation
    cols = _state(oracle, name, shape, ft, dev)
    inv_dz = _inv_dz(shape[1], ft, dev)
    clean = step.fused(inv_dz, cols, 30.0, 2)[0].reshape(4, -1)
    assert bool(torch.isfinite(clean).all())
    rain = 2      # the rain mass output in both schemes
    for flat in (255, 255 + 37):
        assert 0 < flat % shape[1] < shape[1] - 1      # the level below and the level above are in the same column
        for j in (1, 5):
            bad = [c.clone() for c in cols]
            bad[j].view(-1)[flat] = float("nan")
            got = step.fused(inv_dz, bad, 30.0, 2)[0].reshape(4, -1)
            assert bool(torch.isnan(got[:, flat]).all()), (flat, j)
            rest = torch.ones(got.shape[1], dtype=torch.bool, device=dev)
            rest[flat] = False
            if j == 5:
                rest[flat - 1] = False
                assert bool(torch.isnan(got[rain, flat - 1])), flat
                if name == "mp1m":      # per species: cloud liquid, cloud ice and snow of the level below keep their bits
                    assert _eq(got[[0, 1, 3], flat - 1], clean[[0, 1, 3], flat - 1]), flat
            assert _eq(got[:, rest], clean[:, rest]), (flat, j)


def _raw(step, dev, inv_dz, ins, outs, precip, dt, nsub, shape):
    """Through the raw ABI: the columns as they are given (any alignment)."""
    fam = _abi.F32 if step.ft == "f32" else _abi.F64
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    if step.name == "sb2006":
        flags = (_abi.CMX_SB2006_LIMITED if step.mp.is_limited else 0) | step.vel.flag
        _lib.call("cmx_sb2006_column_implicit_average_sedimentation", fam, dev, C.byref(step.mp.c), C.byref(step.tps), C.byref(step.velp),
                  C.byref(step.cloud) if step.cloud is not None else None, flags, dt, nsub, _abi.CMX_STEP_NONNEGATIVE, shape[0], shape[1], p(inv_dz),
                  *[p(t) for t in ins], *[p(t) for t in outs], p(precip[0]))
    else:
        _lib.call("cmx_mp1m_column_implicit_average_sedimentation", fam, dev, C.byref(step.mp.c), C.byref(step.tps), *[C.byref(v) for v in step.vels],
                  step.mp.flags, dt, nsub, _abi.CMX_STEP_NONNEGATIVE, shape[0], shape[1], p(inv_dz), (C.c_void_p * 7)(*[t.data_ptr() for t in ins]),
                  (C.c_void_p * 4)(*[t.data_ptr() for t in outs]), p(precip[0]), p(precip[1]))


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_misaligned_columns_give_the_same_bits(dev, oracle, name, ft):
    """Every column — state, inv_dz, outputs, surface fluxes — is a view that starts one element into its buffer; guard values around the outputs."""
    for shape in ((3, 85), BIG):
        step = Step(name, AC.DEFAULT[name], ft, FLUX[name][1])
        cols = _state(oracle, name, shape, ft, dev)
        inv_dz = _inv_dz(shape[1], ft, dev)
        ref, ref_p = step.fused(inv_dz, cols, 30.0, 2)
        n = shape[0] * shape[1]
        off = lambda t: torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:]  # noqa: E731
        ins, dz = [off(c) for c in cols], off(inv_dz)
        bufs = [torch.full((n + 2,), -7.0, dtype=DT[ft], device=dev) for _ in range(4)]
        pbufs = [torch.full((shape[0] + 2,), -7.0, dtype=DT[ft], device=dev) for _ in range(2)]
        outs, precip = [b[1:-1] for b in bufs], [b[1:-1] for b in pbufs]
        assert all(t.data_ptr() % 16 != 0 for t in ins + outs + precip + [dz])
        _raw(step, dev, dz, ins, outs, precip, 30.0, 2, shape)
        torch.cuda.synchronize()
        assert _eq(torch.stack(outs).reshape(4, *shape), ref) and all(_eq(g, w) for g, w in zip(precip, ref_p))
        assert all(float(b[0]) == float(b[-1]) == -7.0 for b in bufs + pbufs[:len(ref_p)])      # nothing written outside the columns


@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_the_wrappers_refuse_what_the_kernel_cannot_read(dev, oracle, name):
    ft, shape = "f32", (4, 64)
    step = Step(name, AC.DEFAULT[name], ft, FLUX[name][0])
    cols = _state(oracle, name, shape, ft, dev)
    inv_dz = _inv_dz(shape[1], ft, dev)
    step.fused(inv_dz, cols, 30.0, 2)
    # a transposed view of the right shape is refused, not copied; so is a strided one
    tr = [c.clone() for c in cols]
    tr[3] = cols[3].t().contiguous().t()
    assert tr[3].shape == cols[3].shape and not tr[3].is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        step.fused(inv_dz, tr, 30.0, 2)
    wide = [torch.cat([c, c], dim=1)[:, ::2] for c in cols]
    assert wide[0].shape == cols[0].shape
    with pytest.raises(ValueError, match="contiguous"):
        step.fused(inv_dz, wide, 30.0, 2)
    with pytest.raises(ValueError, match="shape"):
        step.fused(inv_dz, [c.reshape(-1) for c in cols], 30.0, 2)
    with pytest.raises(ValueError):
        step.fused(inv_dz, cols[:5] + [cols[5].reshape(shape[1], shape[0])] + cols[6:], 30.0, 2)
    with pytest.raises(ValueError, match="inv_dz"):
        step.fused(inv_dz[:-1], cols, 30.0, 2)
    with pytest.raises(ValueError, match="inv_dz"):
        step.fused(inv_dz.double(), cols, 30.0, 2)
    with pytest.raises((ValueError, TypeError)):
        step.fused(inv_dz, [c.double() for c in cols], 30.0, 2)      # parameter structs of the other float type
    for bad in (dict(dt=-1.0), dict(dt=0.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(nsub=0), dict(nsub=65), dict(nsub=1.5), dict(dt=2e-38, nsub=64)):
        kw = dict(dt=30.0, nsub=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            step.fused(inv_dz, cols, kw["dt"], kw["nsub"])


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_a_captured_call_replays_bit_identically(dev, oracle, name, ft):
    """The entry is a pure launch sequence: captured, replayed once, the same bits."""
    shape = BIG
    step = Step(name, AC.DEFAULT[name], ft, FLUX[name][1])
    cols = _state(oracle, name, shape, ft, dev)
    inv_dz = _inv_dz(shape[1], ft, dev)
    outs = [torch.empty(shape, dtype=DT[ft], device=dev) for _ in range(4)]
    precip = [torch.empty(shape[0], dtype=DT[ft], device=dev) for _ in range(2)]

    def call():
        _raw(step, dev, inv_dz, cols, outs, precip, 30.0, 2, shape)
    eager, eager_p = step.fused(inv_dz, cols, 30.0, 2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for t in outs + precip:
        t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert _eq(torch.stack(outs), eager) and all(_eq(p, w) for p, w in zip(precip, eager_p))


@pytest.mark.parametrize("ft", FTS)
def test_out_of_the_two_moment_wrapper(dev, oracle, ft):
    """Provided outputs are used; a state tensor as an output raises in the wrapper (the step is not in place)."""
    shape = (4, 64)
    step = Step("sb2006", AC.DEFAULT["sb2006"], ft, ("sb", True))
    cols = _state(oracle, "sb2006", shape, ft, dev)
    inv_dz = _inv_dz(shape[1], ft, dev)
    ref, ref_p = step.fused(inv_dz, cols, 30.0, 2)
    out = cmx.ColumnTendencies2M(*[torch.full(shape, -7.0, dtype=DT[ft], device=dev) for _ in range(4)], torch.full((shape[0],), -7.0, dtype=DT[ft], device=dev))
    got, got_p = step.fused(inv_dz, cols, 30.0, 2, out=out)
    assert all(_eq(out[q], ref[q]) and _eq(got[q], ref[q]) for q in range(4)) and _eq(out.precip_flux, ref_p[0]) and got_p[0] is out.precip_flux
    before = [c.clone() for c in cols]
    with pytest.raises(ValueError, match="not in place"):
        step.fused(inv_dz, cols, 30.0, 2, out=cmx.ColumnTendencies2M(cols[3], *out[1:]))
    with pytest.raises(ValueError):
        step.fused(inv_dz, cols, 30.0, 2, out=cmx.ColumnTendencies2M(out[0].to(DT["f32" if ft == "f64" else "f64"]), *out[1:]))      # an output of the other float type
    assert all(_eq(b, c) for b, c in zip(before, cols))
