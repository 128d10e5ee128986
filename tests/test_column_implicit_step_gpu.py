"""The column steps with backward-Euler sedimentation on the device (cmx_sb2006_column_implicit_step_*, cmx_mp1m_column_implicit_step_*;
cmx.column_implicit_step_2m / _1m; include/cmx.h §21):

    G_k = top ? B_k : fma(A_k, G_{k+1}, B_k),     out_k = fma(top ? 0 : G_{k+1}, g, fma(−F_k, g, a_k))·r_k,     surface output G_0

— the degenerate case inv_dz = 0 in bits, the defining identity against the explicit entry of §20, the column budget, positivity at Courant numbers of
several tens (where the explicit entry goes negative), independence of the kernel's chunks and of the other columns, the NaN rule, alignment, graph
capture, `out=` and the wrappers' refusals.  Both schemes, both float types, the option cases of implicit_average_cases.CASES, the flux options of the §20
test; the shapes sit around the kernel's chunk of 256 points and the column top, (2, 600) has columns of three chunks.  No call has more than 4 200 points.
The Float64 recipe and the bounds, with their derivations: tests/column_implicit_step_cases.py (self-checked in tests/test_column_implicit_step_host.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import column_implicit_step_cases as SC
import implicit_average_cases as AC
import test_column_implicit_average_gpu as IA      # the §20 test's Step (entries and flux options), states and inv_dz generator
import cmx
from cmx import _abi, _lib

pytestmark = pytest.mark.gpu
DT, EPS, FTS, FLUX = IA.DT, SC.EPS, IA.FTS, IA.FLUX
_eq, _inv_dz, _state = IA._eq, IA._inv_dz, IA._state
BIG, LONG = (65, 63), (2, 600)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class Step(IA.Step):
    """… plus the implicit step and the fall speeds of the existing velocity entries."""

    def implicit(self, inv_dz, cols, dt, nsub, nonneg=True, **kw):
        """([4, n_col, n_lev] outputs, the surface fluxes)"""
        if self.name == "sb2006":
            r = cmx.column_implicit_step_2m(self.mp, self.tps, inv_dz, *cols, dt, nsub, nonneg, vel=self.vel, vel_params=self.velp, cloud_vel=self.cloud,
                                            want_precip_flux=True, **kw)
            return torch.stack(list(r[:4])), [r.precip_flux]
        r = cmx.column_implicit_step_1m(self.mp, self.tps, *self.vels, inv_dz, *cols, dt, nsub, nonneg, **kw)
        return torch.stack(list(r[:4])), [r.precip_rai, r.precip_sno]

    def velocities(self, cols):
        """[4, n_col, n_lev] fall speeds in the order of the outputs, from the existing velocity entries on the clamped states (the fluxes are those of
        ρ⁺, χ⁺): cmx.sedimentation_velocities; the rain velocities of the tendencies entry and cmx.cloud_terminal_velocity (0 without cloud sedimentation)."""
        shape = cols[0].shape
        flat = [c.reshape(-1) for c in cols]
        pos = [flat[0].clamp(min=0), flat[1], flat[2]] + [c.clamp(min=0) for c in flat[3:]]
        if self.name == "mp1m":
            w = cmx.sedimentation_velocities(self.mp, *self.vels, pos[0], *pos[3:])
            return torch.stack(list(w)).reshape(4, *shape)
        r = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), self.mp, self.tps, *pos, vel=self.vel, vel_params=self.velp)
        zero = torch.zeros_like(flat[0])
        w = [zero, zero, r.vt_rai_m, r.vt_rai_n]
        if self.cloud is not None:
            cv = cmx.cloud_terminal_velocity(self.mp.c.seifert_beheng.pdf_c, self.cloud, pos[3], pos[0], pos[0] * pos[4])
            w[0], w[1] = cv.vt_m, cv.vt_n
        return torch.stack(w).reshape(4, *shape)


def _np(t):
    return t.double().cpu().numpy()


def _nonneg(cols):
    """Non-negative states: ρ and the four species clamped at 0."""
    return [cols[0].clamp(min=0), cols[1], cols[2]] + [c.clamp(min=0) for c in cols[3:]]


def _at_or_below_a_nonfinite_average(step, a):
    """[4, n_col, n_lev] mask: the elements of a FALLING species at or below a level where its average is not finite, in the same column."""
    bad = ~torch.isfinite(a)
    if step.name == "sb2006" and step.cloud is None:
        bad[:2] = False      # q_lcl and n_lcl do not fall: their outputs are the averages themselves
    return bad.flip(-1).cumsum(-1).flip(-1) > 0


def _quiet_surface(name, cols):
    """The states with level 0 of every column replaced by a point whose precipitating species have a = 0: rain (different in every column) in strongly
    supersaturated warm air with no cloud, no ice and no snow — nothing forms, collects, evaporates, melts or freezes rain mass, and there is no snow."""
    out = [c.clone() for c in cols]
    n_col = cols[0].shape[0]
    ramp = torch.linspace(1.0, 2.0, n_col, dtype=cols[0].dtype, device=cols[0].device)
    out[0][:, 0], out[1][:, 0], out[2][:, 0] = 1.0, 290.0, 0.05
    out[3][:, 0], out[4][:, 0] = 0.0, 0.0
    if name == "sb2006":
        out[5][:, 0], out[6][:, 0] = 2e-4 * ramp, 2e4 * ramp
    else:
        out[5][:, 0], out[6][:, 0] = 2e-4 * ramp, 0.0
    return out


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_without_levels_the_step_is_the_average_entry_in_every_bit(dev, oracle, name, case, ft):
    """inv_dz ≡ 0: c = 0, r = 1 exactly, g = 0 — the four outputs are the average entry's on the flattened states for every Δt, nsub, limiter setting and shape
    (the flux options rotate over the shapes).  This is also where F is shown to have the bits of the existing flux functions: G_0 = fma(β, a, F)·1, so with
    a = 0 at level 0 (a rain point in supersaturated air without cloud, ice or snow) the surface fluxes are the existing column entry's F_0 in every bit.
    Where an average is not finite — without the limiter, at Δt = 300 s, the substeps diverge at a few of these states — the rule of §21 applies on top: the
    recurrence carries it to the lower levels of that falling species (0·Inf and fma(NaN, 0, ·) are NaN), which are then required to be non-finite instead;
    every other element, the non-falling species included, has the average entry's bits.  With the limiter there is no such element."""
    nonzero = carried = 0
    for k, shape in enumerate(SC.SHAPES):
        step = Step(name, case, ft, FLUX[name][k % len(FLUX[name])])
        cols = _state(oracle, name, shape, ft, dev)
        IA._assert_regular(cols)
        zero = _inv_dz(shape[1], ft, dev, zero=True)
        for dt in SC.DTS:
            for nsub in AC.NSUBS:
                for nonneg in (True, False):
                    got, _ = step.implicit(zero, cols, dt, nsub, nonneg)
                    want = step.average(cols, dt, nsub, nonneg)
                    lost = _at_or_below_a_nonfinite_average(step, want)
                    carried += int(lost.sum())
                    assert _eq(got[~lost], want[~lost]), (shape, step.flux, dt, nsub, nonneg, int(((got != want) & ~(torch.isnan(got) & torch.isnan(want)) & ~lost).sum()))
                    assert not bool(torch.isfinite(got[lost]).any()), (shape, step.flux, dt, nsub, nonneg)
                    assert nonneg is False or not bool(lost.any())      # with the limiter every average of these states is finite
        quiet = _quiet_surface(name, cols)
        precip = [2] if name == "sb2006" else [2, 3]
        for dt, nsub in ((1.0, 1), (300.0, 2)):
            # the arrangement: a = 0 for the species whose surface flux is an output; the columns where the average is not exactly 0 are left out
            still = (step.average(quiet, dt, nsub)[:, :, 0][precip] == 0).all(0)
            got, want = step.implicit(zero, quiet, dt, nsub)[1], step.column(zero, quiet)[1]
            for g, w in zip(got, want):
                assert g.shape == (shape[0],) and _eq(g[still], w[still]) and bool(torch.isfinite(w).all()), (shape, step.flux, dt)
            nonzero += int((want[0][still] > 0).sum())
    print(f"{name} {case} {ft}: {nonzero} positive surface rain fluxes compared in bits; {carried} elements at or below a non-finite average")
    assert nonzero >= sum(s[0] for s in SC.SHAPES)      # at least one (Δt, nsub) per column: the comparison is not one of zeros


def _terms(step, step_dev_cols, inv_dz, dt, nsub):
    """Everything the host-side properties need, as Float64 arrays: out, G_0 per precipitating species, out_expl, F_0 of the explicit entry, a, w, ρ, χ."""
    cols = step_dev_cols
    out, G0 = step.implicit(inv_dz, cols, dt, nsub)
    expl, F0 = step.fused(inv_dz, cols, dt, nsub)
    return dict(out=_np(out), G0=[_np(p) for p in G0], expl=_np(expl), F0=[_np(p) for p in F0], a=_np(step.average(cols, dt, nsub)),
                w=_np(step.velocities(cols)), rho=_np(cols[0]), chi=np.stack([_np(c) for c in cols[3:]]), inv_dz=_np(inv_dz))


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_the_defining_identity_against_the_explicit_entry(dev, oracle, name, case, ft):
    """For every k and j, in Float64 on the host:  out_k (1 + c_k) − out_expl_k = g_k β_{k+1} out_{k+1}  (top: right side 0), and at the surface
    G_0 = F_0 + β_0 out_0 with F_0 the explicit entry's surface flux.  out_expl: the §20 entry on the same inputs; c, β from the fall speeds of the existing
    velocity entries on the same states.  With the top condition this triangular set pins every output.  Bound: M_IDENTITY·eps(FT)·S per element, S the sum
    of the magnitudes of the terms — the count of roundings is in tests/column_implicit_step_cases.py; it includes 3·W_ULP for the difference between the
    velocity entries' w and the in-kernel w, which was measured first (Float64 device run, n_lev = 1, inv_dz = 1: the explicit entry gives F/ρ⁺ = a − out_expl,
    so χ⁺ w = a − out_expl wherever F/ρ⁺ exceeds 1000 |a|): at most 2.9 eps (SB2006) and 1.8 eps (1-moment), figures that contain the rounding of g too; W_ULP = 3.
    No state is set aside; sedimentation moved at least a quarter of the elements."""
    total = moved = 0
    for k, shape in enumerate(SC.SHAPES):
        step = Step(name, case, ft, FLUX[name][k % len(FLUX[name])])
        cols = _state(oracle, name, shape, ft, dev)
        inv_dz = _inv_dz(shape[1], ft, dev)
        for dt in SC.DTS:
            t = _terms(step, cols, inv_dz, dt, 2)
            rp = np.maximum(t["rho"], 0.0)[None]
            idz = t["inv_dz"][None, None, :]
            c, beta, g = dt * t["w"] * idz, dt * t["w"] * rp, idz / rp
            F = rp * np.maximum(t["chi"], 0.0) * t["w"]      # for the scale only
            assert np.isfinite(t["out"]).all() and np.isfinite(t["expl"]).all()
            res, S = SC.identity(t["out"], t["expl"], t["a"], F, c, beta, g)
            worst = float((res / np.maximum(S, 1e-300)).max() / EPS[ft])
            prec = [2] if name == "sb2006" else [2, 3]
            sres, ssc = zip(*[SC.surface(G0, F0, beta[j, :, 0], t["out"][j, :, 0]) for j, G0, F0 in zip(prec, t["G0"], t["F0"])])
            sworst = max(float((r / np.maximum(s, 1e-300)).max()) for r, s in zip(sres, ssc)) / EPS[ft]
            print(f"{name} {case} {ft} {shape} {step.flux} dt={dt:g}: c max {c.max():.3g}, identity {worst:.3g} eps S, surface {sworst:.3g} eps")
            assert bool((res <= SC.M_IDENTITY * EPS[ft] * S).all()), (shape, step.flux, dt, worst)
            assert all(bool((r <= SC.M_IDENTITY * EPS[ft] * s).all()) for r, s in zip(sres, ssc)), (shape, step.flux, dt, sworst)
            if dt == 30.0:
                total += t["out"].size
                moved += int((np.abs(t["out"] - t["a"]) > 0).sum())
    print(f"{name} {case} {ft}: sedimentation moved {moved} of {total} elements")
    assert moved >= total / 4, (moved, total)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_the_column_budget_closes(dev, oracle, name, case, ft):
    """In Float64 on the host, per column and precipitating species (those whose G_0 is an output): Σ_k ρ_k out_k/inv_dz_k + G_0 = Σ_k ρ_k a_k/inv_dz_k
    within M_BUDGET·eps(FT)·(Σ ρ|out|/inv_dz + |G_0|); the count is in tests/column_implicit_step_cases.py."""
    for k, shape in enumerate(SC.SHAPES):
        step = Step(name, case, ft, FLUX[name][(k + 2) % len(FLUX[name])])
        cols = _state(oracle, name, shape, ft, dev)
        inv_dz = _inv_dz(shape[1], ft, dev)
        prec = [2] if name == "sb2006" else [2, 3]
        for dt in SC.DTS:
            out, G0 = step.implicit(inv_dz, cols, dt, 2)
            a = _np(step.average(cols, dt, 2))
            res, sc = SC.budget(_np(out)[prec], np.stack([_np(p) for p in G0]), a[prec], _np(cols[0]), _np(inv_dz))
            worst = float((res / np.maximum(sc, 1e-300)).max() / EPS[ft])
            print(f"{name} {case} {ft} {shape} {step.flux} dt={dt:g}: budget residual {worst:.3g} eps")
            assert bool((res <= SC.M_BUDGET * EPS[ft] * sc).all()), (shape, step.flux, dt, worst)


# The share of cells with c > 1 that the explicit entry of §20 leaves negative in a falling species at Δt = 300 s.  Counted first on an MI355X for these
# states: 3 675 – 4 678 of 8 582 – 9 609 cells (43 – 49 %) in every scheme, option case and float type; the floor asserted is well below that.
EXPLICIT_NEGATIVE_FLOOR = 0.2


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_positivity_at_large_courant_numbers(dev, oracle, name, case, ft):
    """nonnegative = True, non-negative states, Δt = 300 s: χ_k + Δt out_k ≥ −m_k·eps(FT)·(χ_k + Δt|a_k| + Δt g_k (F_k + max_{l>k}(F_l + β_l|a_l|))), m_k counted
    in column_implicit_step_cases.m_positivity (rounding in G is relative to the content of the cells above and compounds down the chain, contracting by
    c/(1 + c) per level: m_k = 7 + 5·min(levels above, 1 + the largest c above)); the worst ratio against m = 1 is printed.  On the same inputs
    the explicit entry of §20 leaves a falling species negative in a non-trivial share of the cells with c > 1: the regime the step exists for."""
    cells = negative = 0
    worst1 = 0.0
    for k, shape in enumerate(SC.SHAPES):
        step = Step(name, case, ft, FLUX[name][(k + 1) % len(FLUX[name])])
        cols = _nonneg(_state(oracle, name, shape, ft, dev))
        inv_dz = _inv_dz(shape[1], ft, dev)
        dt = 300.0
        t = _terms(step, cols, inv_dz, dt, 2)
        rp = t["rho"][None]
        idz = t["inv_dz"][None, None, :]
        c, beta, g = dt * t["w"] * idz, dt * t["w"] * rp, idz / rp
        F = rp * t["chi"] * t["w"]
        new, sc = SC.positivity(t["chi"], t["out"], t["a"], F, beta, g, dt)
        m = SC.m_positivity(c)
        worst = float((-new / np.maximum(sc, 1e-300) / m).max() / EPS[ft])
        worst1 = max(worst1, float((-new / np.maximum(sc, 1e-300)).max() / EPS[ft]))
        fast = c > 1.0
        neg = fast & (t["chi"] + dt * t["expl"] < 0)
        cells += int(fast.sum())
        negative += int(neg.sum())
        print(f"{name} {case} {ft} {shape} {step.flux}: c max {c.max():.3g}, worst −(χ + Δt out)/(m eps scale) {worst:.3g}; explicit: {int(neg.sum())} of {int(fast.sum())} cells with c > 1 negative")
        assert bool((new >= -m * EPS[ft] * sc).all()), (shape, step.flux, worst)
    print(f"{name} {case} {ft}: the explicit entry leaves {negative} of {cells} cells with c > 1 negative; worst −(χ + Δt out)/(eps scale), i.e. against m = 1: {worst1:.3g}")
    assert cells > 500 and negative >= EXPLICIT_NEGATIVE_FLOOR * cells, (negative, cells)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_results_do_not_depend_on_chunks_or_other_columns(dev, oracle, name, case, ft):
    """EVERY column run alone equals its row of the full call; the first m columns of a call equal the call on those columns; (2, 600) as two calls of
    (1, 600); NaNs filling one column leave every other column's bits alone — the column stored before it and the one stored after it in particular.
    What makes this a comparison of two different chunkings: a workgroup owns 16 columns of (65, 63) — 1008 points, chunk edges at 256, 512 and 768 from its
    first point — so the columns at positions 4, 8 and 12 of a workgroup (columns 4, 8, 12, 20, …) straddle a chunk edge in the full call and take their G
    across it through the carry, while alone, or as the last columns of a prefix of 5 or 13, they sit in other chunks; of (5, 300) a workgroup owns three
    columns (chunk edges inside columns 0, 1 and 2), while a column alone starts its own chunks.  Those columns are among the ones filled with NaN too."""
    for k, shape in enumerate([(3, 85), (4, 64), BIG, (5, 300), LONG]):
        step = Step(name, case, ft, FLUX[name][(k + 1) % len(FLUX[name])])
        cols = _state(oracle, name, shape, ft, dev)
        inv_dz = _inv_dz(shape[1], ft, dev)
        full, precip = step.implicit(inv_dz, cols, 300.0, 2)
        for c in range(shape[0]):
            alone, p = step.implicit(inv_dz, [x[c:c + 1].contiguous() for x in cols], 300.0, 2)
            assert _eq(alone[:, 0], full[:, c]) and all(_eq(pa[0], pf[c]) for pa, pf in zip(p, precip)), (shape, c)
        for m in sorted({1, 2, 5, 13, 21, shape[0] - 1} & set(range(1, shape[0]))):
            head, p = step.implicit(inv_dz, [x[:m].contiguous() for x in cols], 300.0, 2)
            assert _eq(head, full[:, :m]) and all(_eq(pa, pf[:m]) for pa, pf in zip(p, precip)), (shape, m)
            tail, p = step.implicit(inv_dz, [x[shape[0] - m:].contiguous() for x in cols], 300.0, 2)      # other positions in the workgroups
            assert _eq(tail, full[:, shape[0] - m:]) and all(_eq(pa, pf[shape[0] - m:]) for pa, pf in zip(p, precip)), (shape, -m)
        for c in sorted({0, 1, 4, 8, 20, shape[0] - 1} & set(range(shape[0]))):
            bad = [x.clone() for x in cols]
            for x in bad:
                x[c] = float("nan")
            got, p = step.implicit(inv_dz, bad, 300.0, 2)
            keep = torch.arange(shape[0], device=dev) != c
            assert bool(torch.isnan(got[:, c]).all()) and _eq(got[:, keep], full[:, keep]), (shape, c)
            assert all(_eq(pa[keep], pf[keep]) and bool(torch.isnan(pa[c])) for pa, pf in zip(p, precip)), (shape, c)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_every_flux_has_the_bits_of_the_existing_flux_functions(dev, oracle, name, case, ft):
    """All four species, every state, every flux option: columns of ONE level with inv_dz = 1 and a Δt so small that 1 + c rounds to 1 (c = Δt·w < eps/2 for
    every fall speed below 50 m/s), hence r = 1 exactly and, every point being a top, out = fma(−F, g, a) — the explicit entry's expression on the same a and
    g, whose flux term χ w dominates a.  The outputs then agree in every bit exactly if the new (F, w) functions form F as the flux-only functions do."""
    dt = {"f32": 1e-9, "f64": 1e-18}[ft]
    assert 50.0 * dt < EPS[ft] / 2
    shape = (4200, 1)
    cols = _state(oracle, name, shape, ft, dev)
    one = torch.ones(1, dtype=DT[ft], device=dev)
    differ = 0
    for flux in FLUX[name]:
        step = Step(name, case, ft, flux)
        assert float(step.velocities(cols).max()) < 50.0
        got, want = step.implicit(one, cols, dt, 1)[0], step.fused(one, cols, dt, 1)[0]
        assert _eq(got, want), (flux, int(((got != want) & ~(torch.isnan(got) & torch.isnan(want))).sum()))
        differ += int((want != step.average(cols, dt, 1)).sum())
    assert differ > 4200      # the flux term is there: the outputs are not the averages


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_the_nan_rule(dev, oracle, name, case, ft):
    """A NaN in T or in q_rai at (col, k): the averages of the point are NaN (§19), so all four B are, and the recurrence carries the NaN down — all four
    outputs are NaN at the levels ≤ k of that column and the column's surface fluxes are NaN; the levels > k and the other columns keep their bits.  (With a
    NaN in q_rai the rain flux of the point is NaN too; that the other 1-moment species could keep their bits below the point, as they do in §20, does not
    survive the rule of §21: their a is NaN at the point.)  With cloud sedimentation for SB2006, so that all four species fall.  The NaN sits at a chunk edge
    and inside a chunk; for (2, 600) also in a column's top chunk, so that the carry is what transports it across two chunk boundaries."""
    for shape, flats in ((BIG, (255, 256, 255 + 37)), (LONG, (600 + 599, 600 + 512, 600 + 511, 600 + 300, 255))):
        step = Step(name, case, ft, FLUX[name][1])
        cols = _state(oracle, name, shape, ft, dev)
        inv_dz = _inv_dz(shape[1], ft, dev)
        clean, clean_p = step.implicit(inv_dz, cols, 300.0, 2)
        assert bool(torch.isfinite(clean).all())
        for flat in flats:
            col, lev = divmod(flat, shape[1])
            for j in (1, 5):
                bad = [c.clone() for c in cols]
                bad[j].view(-1)[flat] = float("nan")
                got, got_p = step.implicit(inv_dz, bad, 300.0, 2)
                hit = torch.zeros(shape, dtype=torch.bool, device=dev)
                hit[col, :lev + 1] = True
                assert bool(torch.isnan(got[:, hit]).all()), (shape, flat, j)
                assert _eq(got[:, ~hit], clean[:, ~hit]), (shape, flat, j)
                other = torch.arange(shape[0], device=dev) != col
                assert all(bool(torch.isnan(p[col])) and _eq(p[other], q[other]) for p, q in zip(got_p, clean_p)), (shape, flat, j)


def _raw(step, dev, inv_dz, ins, outs, precip, dt, nsub, shape):
    """Through the raw ABI: the columns as they are given (any alignment)."""
    fam = _abi.F32 if step.ft == "f32" else _abi.F64
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    if step.name == "sb2006":
        flags = (_abi.CMX_SB2006_LIMITED if step.mp.is_limited else 0) | step.vel.flag
        _lib.call("cmx_sb2006_column_implicit_step", fam, dev, C.byref(step.mp.c), C.byref(step.tps), C.byref(step.velp),
                  C.byref(step.cloud) if step.cloud is not None else None, flags, dt, nsub, _abi.CMX_STEP_NONNEGATIVE, shape[0], shape[1], p(inv_dz),
                  *[p(t) for t in ins], *[p(t) for t in outs], p(precip[0]))
    else:
        _lib.call("cmx_mp1m_column_implicit_step", fam, dev, C.byref(step.mp.c), C.byref(step.tps), *[C.byref(v) for v in step.vels],
                  step.mp.flags, dt, nsub, _abi.CMX_STEP_NONNEGATIVE, shape[0], shape[1], p(inv_dz), (C.c_void_p * 7)(*[t.data_ptr() for t in ins]),
                  (C.c_void_p * 4)(*[t.data_ptr() for t in outs]), p(precip[0]), p(precip[1]))


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_misaligned_columns_give_the_same_bits(dev, oracle, name, ft):
    """Every column — state, inv_dz, outputs, surface fluxes — is a view that starts one element into its buffer; guard values around the outputs."""
    for shape in ((3, 85), BIG, LONG):
        step = Step(name, AC.DEFAULT[name], ft, FLUX[name][1])
        cols = _state(oracle, name, shape, ft, dev)
        inv_dz = _inv_dz(shape[1], ft, dev)
        ref, ref_p = step.implicit(inv_dz, cols, 300.0, 2)
        n = shape[0] * shape[1]
        off = lambda t: torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:]  # noqa: E731
        ins, dz = [off(c) for c in cols], off(inv_dz)
        bufs = [torch.full((n + 2,), -7.0, dtype=DT[ft], device=dev) for _ in range(4)]
        pbufs = [torch.full((shape[0] + 2,), -7.0, dtype=DT[ft], device=dev) for _ in range(2)]
        outs, precip = [b[1:-1] for b in bufs], [b[1:-1] for b in pbufs]
        assert all(t.data_ptr() % 16 != 0 for t in ins + outs + precip + [dz])
        _raw(step, dev, dz, ins, outs, precip, 300.0, 2, shape)
        torch.cuda.synchronize()
        assert _eq(torch.stack(outs).reshape(4, *shape), ref) and all(_eq(g, w) for g, w in zip(precip, ref_p))
        assert all(float(b[0]) == float(b[-1]) == -7.0 for b in bufs + pbufs[:len(ref_p)])      # nothing written outside the columns


@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_the_wrappers_refuse_what_the_kernel_cannot_read(dev, oracle, name):
    ft, shape = "f32", (4, 64)
    step = Step(name, AC.DEFAULT[name], ft, FLUX[name][0])
    cols = _state(oracle, name, shape, ft, dev)
    inv_dz = _inv_dz(shape[1], ft, dev)
    step.implicit(inv_dz, cols, 30.0, 2)
    # a transposed view of the right shape is refused, not copied; so is a strided one
    tr = [c.clone() for c in cols]
    tr[3] = cols[3].t().contiguous().t()
    assert tr[3].shape == cols[3].shape and not tr[3].is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        step.implicit(inv_dz, tr, 30.0, 2)
    wide = [torch.cat([c, c], dim=1)[:, ::2] for c in cols]
    assert wide[0].shape == cols[0].shape
    with pytest.raises(ValueError, match="contiguous"):
        step.implicit(inv_dz, wide, 30.0, 2)
    with pytest.raises(ValueError, match="shape"):
        step.implicit(inv_dz, [c.reshape(-1) for c in cols], 30.0, 2)
    with pytest.raises(ValueError):
        step.implicit(inv_dz, cols[:5] + [cols[5].reshape(shape[1], shape[0])] + cols[6:], 30.0, 2)
    with pytest.raises(ValueError, match="inv_dz"):
        step.implicit(inv_dz[:-1], cols, 30.0, 2)
    with pytest.raises(ValueError, match="inv_dz"):
        step.implicit(inv_dz.double(), cols, 30.0, 2)
    with pytest.raises((ValueError, TypeError)):
        step.implicit(inv_dz, [c.double() for c in cols], 30.0, 2)      # parameter structs of the other float type
    for bad in (dict(dt=-1.0), dict(dt=0.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(nsub=0), dict(nsub=65), dict(nsub=1.5), dict(dt=2e-38, nsub=64)):
        kw = dict(dt=30.0, nsub=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            step.implicit(inv_dz, cols, kw["dt"], kw["nsub"])


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_a_captured_call_replays_bit_identically(dev, oracle, name, ft):
    """The entry is a pure launch sequence — one kernel, no parallel branches: captured, replayed once, the same bits."""
    shape = LONG
    step = Step(name, AC.DEFAULT[name], ft, FLUX[name][1])
    cols = _state(oracle, name, shape, ft, dev)
    inv_dz = _inv_dz(shape[1], ft, dev)
    outs = [torch.empty(shape, dtype=DT[ft], device=dev) for _ in range(4)]
    precip = [torch.empty(shape[0], dtype=DT[ft], device=dev) for _ in range(2)]

    def call():
        _raw(step, dev, inv_dz, cols, outs, precip, 300.0, 2, shape)
    eager, eager_p = step.implicit(inv_dz, cols, 300.0, 2)
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
    ref, ref_p = step.implicit(inv_dz, cols, 30.0, 2)
    out = cmx.ColumnTendencies2M(*[torch.full(shape, -7.0, dtype=DT[ft], device=dev) for _ in range(4)], torch.full((shape[0],), -7.0, dtype=DT[ft], device=dev))
    got, got_p = step.implicit(inv_dz, cols, 30.0, 2, out=out)
    assert all(_eq(out[q], ref[q]) and _eq(got[q], ref[q]) for q in range(4)) and _eq(out.precip_flux, ref_p[0]) and got_p[0] is out.precip_flux
    before = [c.clone() for c in cols]
    with pytest.raises(ValueError, match="not in place"):
        step.implicit(inv_dz, cols, 30.0, 2, out=cmx.ColumnTendencies2M(cols[3], *out[1:]))
    with pytest.raises(ValueError):
        step.implicit(inv_dz, cols, 30.0, 2, out=cmx.ColumnTendencies2M(out[0].to(DT["f32" if ft == "f64" else "f64"]), *out[1:]))      # an output of the other float type
    assert all(_eq(b, c) for b, c in zip(before, cols))
