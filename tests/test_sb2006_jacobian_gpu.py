"""The SB2006 warm-rain Jacobian on the device (cmx_sb2006_warm_rain_jacobian_*, cmx.warm_rain_jacobian_2m): the parity assertions of
tests/test_sb2006_jacobian_host.py through the kernel (same states, same finite-difference reference of the Float64 oracle, same bounds, same 1 % condition —
tests/jacobian_cases.py — in both of its measures: the per-row one of the reference and the input-scaled one, which resolves the T, n_lcl and n_rai columns;
worst input-scaled value on the device 2.3e-8 in Float64 and 5.3e-6 in Float32, the Float32 T column ≤ 2.9e-6), the primal against cmx.bulk_microphysics_tendencies bit for bit, column selection, the edges of the launch path, the NaN rule and
graph capture.  No shape is larger than 4096 points."""
import ctypes as C

import numpy as np
import pytest
import torch

import jacobian_cases as JC
import cmx
from cmx import _abi, _lib, synthetic
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _dev_cols(cols, ft, dev):
    return [torch.from_numpy(np.array(c, dtype=np.float64)).to(DT[ft]).to(dev) for c in cols]      # (a copy: the shared reference columns are read-only)


def _eq(a, b):
    """Same bits, NaN = NaN."""
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


# ---- parity -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("limited,perturbed", [(True, False), (False, False), (True, True)])
def test_jacobian_matches_central_differences_of_the_oracle(dev, oracle, ft, limited, perturbed):
    """Float64: every row of every kept state inside the reference's own 1e-5 (test/ad_compat_tests.jl:163).  Float32 against the same Float64 reference:
    every row inside 1e-3, except dn_rai_dt with the perturbed parameter set (2.3e-3 at one state), held entry by entry to jacobian_cases.float32_bound.
    Input-scaled measure: every (row, column) inside the same 1e-5 / 1e-3, no exception.  The perturbed parameter set runs the general-exponent instantiation."""
    wr = JC.warm_rain_params(ft, limited, JC.perturbed_overrides() if perturbed else None)
    tps = P.ThermodynamicsParameters(ft)
    for which in ("interior", "points"):
        cols = _dev_cols(JC.reference(limited, perturbed, which)[0], ft, dev)
        r = cmx.warm_rain_jacobian_2m(wr, tps, *cols)
        assert r.tendencies is None and r.wrt == JC.WRT and r.jac.shape == (4, 6, cols[0].numel()) and r.jac.is_contiguous()
        JC.assert_parity(ft, r.jac.cpu().numpy(), limited, perturbed, which, "device")


# ---- the primal ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("limited", [True, False])
def test_tendencies_are_bit_identical_to_the_tendencies_entry(dev, oracle, ft, limited):
    """with_tendencies=True gives the columns of cmx.bulk_microphysics_tendencies on the same tensors, bit for bit, on the interior set and on the broad
    synthetic set (zeros, negative values, every gate); on the latter every Jacobian entry is finite wherever the four tendencies are."""
    wr, tps = P.WarmRainParams2M(ft, limited), P.ThermodynamicsParameters(ft)
    for name, cols in (("interior", _dev_cols(JC.reference(limited)[0], ft, dev)), ("synthetic", list(synthetic.sb2006_state(4096, dtype=DT[ft], device=dev)))):
        want = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), wr, tps, *cols)
        for wrt in (JC.WRT, ("n_rai", "q_tot"), ()):
            r = cmx.warm_rain_jacobian_2m(wr, tps, *cols, wrt=wrt, with_tendencies=True)
            for o in range(4):
                assert _eq(r.tendencies[o], want[o]), (name, wrt, JC.OUT[o])
        r = cmx.warm_rain_jacobian_2m(wr, tps, *cols, with_tendencies=True)
        finite = torch.isfinite(r.tendencies).all(dim=0)
        assert finite.sum() > 0.9 * finite.numel()
        assert bool(torch.isfinite(r.jac[:, :, finite]).all()), name


# ---- column selection ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_a_subset_in_any_order_gives_the_columns_of_the_full_call(dev, oracle, ft):
    wr, tps = P.WarmRainParams2M(ft, True), P.ThermodynamicsParameters(ft)
    cols = [c[:1000].contiguous() for c in _dev_cols(JC.reference(True)[0], ft, dev)]
    full = cmx.warm_rain_jacobian_2m(wr, tps, *cols).jac
    # sizes 1 … 5: below, at and above the tangents per pass (3 in both float types: csrc/cmx_sb2006_jacobian.hpp), multiples of it and not
    for wrt in (("q_rai",), ("n_rai", "T"), ("q_lcl", "T", "n_lcl"), ("n_rai", "q_rai", "n_lcl", "q_tot"), ("q_rai", "q_tot", "n_lcl", "T", "q_lcl"),
                tuple(reversed(JC.WRT))):
        r = cmx.warm_rain_jacobian_2m(wr, tps, *cols, wrt=wrt)
        assert r.jac.shape == (4, len(wrt), 1000) and r.wrt == wrt
        for k, name in enumerate(wrt):
            assert _eq(r.jac[:, k], full[:, JC.WRT.index(name)]), (wrt, name)


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_a_null_member_of_a_row_leaves_the_other_members_unchanged(dev, oracle, ft):
    """The raw ABI: any of the 24 column pointers may be NULL; a column that is written does not depend on which others are."""
    wr, tps = P.WarmRainParams2M(ft, True), P.ThermodynamicsParameters(ft)
    cols = [c[:257].contiguous() for c in _dev_cols(JC.reference(True)[0], ft, dev)]
    full = cmx.warm_rain_jacobian_2m(wr, tps, *cols).jac
    rng = np.random.default_rng(3)
    for trial in range(3):
        wanted = rng.random((4, 6)) < 0.5
        wanted[trial, :] = [True, False, True, False, False, True]
        got = torch.full((4, 6, 257), -7.0, dtype=DT[ft], device=dev)
        ptrs = (C.c_void_p * 24)(*[got[o, j].data_ptr() if wanted[o, j] else None for o in range(4) for j in range(6)])
        _lib.call("cmx_sb2006_warm_rain_jacobian", _abi.F32 if ft == "f32" else _abi.F64, dev, C.byref(wr.c), C.byref(tps), _abi.CMX_SB2006_LIMITED, 257,
                  *[C.c_void_p(c.data_ptr()) for c in cols], ptrs, None)
        torch.cuda.synchronize()
        for o in range(4):
            for j in range(6):
                if wanted[o, j]:
                    assert _eq(got[o, j], full[o, j]), (trial, o, j)
                else:
                    assert bool((got[o, j] == -7.0).all()), (trial, o, j)


# ---- the edges of the launch path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_sizes_alignment_and_the_empty_call(dev, oracle, ft):
    wr, tps = P.WarmRainParams2M(ft, True), P.ThermodynamicsParameters(ft)
    base = _dev_cols(JC.reference(True)[0], ft, dev)
    ref = cmx.warm_rain_jacobian_2m(wr, tps, *base, with_tendencies=True)
    for n in (1, 63, 64, 65, 257, 1000):
        r = cmx.warm_rain_jacobian_2m(wr, tps, *[c[:n].contiguous() for c in base], with_tendencies=True)
        assert _eq(r.jac, ref.jac[:, :, :n]) and _eq(r.tendencies, ref.tendencies[:, :n]), n
        # inputs and outputs as views offset by one element: no column starts on a 16-byte boundary
        shifted = [torch.cat([c[:1], c[:n]])[1:] for c in base]
        jbuf = torch.full((1 + 24 * n + 1,), -7.0, dtype=DT[ft], device=dev)
        tbuf = torch.full((1 + 4 * n + 1,), -7.0, dtype=DT[ft], device=dev)
        out = (jbuf[1:1 + 24 * n].view(4, 6, n), tbuf[1:1 + 4 * n].view(4, n))
        assert all(s.data_ptr() % 16 != 0 for s in shifted) and out[0].data_ptr() % 16 != 0 and out[1].data_ptr() % 16 != 0
        r = cmx.warm_rain_jacobian_2m(wr, tps, *shifted, with_tendencies=True, out=out)
        assert r.jac.data_ptr() == out[0].data_ptr()
        assert _eq(r.jac, ref.jac[:, :, :n]) and _eq(r.tendencies, ref.tendencies[:, :n]), n
        assert float(jbuf[0]) == float(jbuf[-1]) == float(tbuf[0]) == float(tbuf[-1]) == -7.0      # nothing written outside the columns
    # n = 0 returns without touching memory (and before the columns are looked at)
    guard = torch.full((8,), -7.0, dtype=DT[ft], device=dev)
    empty = [guard[4:4] for _ in range(7)]
    r = cmx.warm_rain_jacobian_2m(wr, tps, *empty, with_tendencies=True, out=(guard[4:4].view(4, 6, 0), guard[4:4].view(4, 0)))
    torch.cuda.synchronize()
    assert r.jac.numel() == 0 and bool((guard == -7.0).all())


# ---- the NaN rule -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_a_nan_input_poisons_every_output_of_its_point_only(dev, oracle, ft):
    wr, tps = P.WarmRainParams2M(ft, True), P.ThermodynamicsParameters(ft)
    cols = [c[:130].contiguous() for c in _dev_cols(JC.reference(True)[0], ft, dev)]
    clean = cmx.warm_rain_jacobian_2m(wr, tps, *cols, with_tendencies=True)
    others = torch.arange(130, device=dev) != 77
    for j in range(7):
        bad = [c.clone() for c in cols]
        bad[j][77] = float("nan")
        r = cmx.warm_rain_jacobian_2m(wr, tps, *bad, with_tendencies=True)
        assert bool(torch.isnan(r.jac[:, :, 77]).all()) and bool(torch.isnan(r.tendencies[:, 77]).all()), j
        assert _eq(r.jac[:, :, others], clean.jac[:, :, others]) and _eq(r.tendencies[:, others], clean.tendencies[:, others]), j


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_captured_call_replays_bit_identically(dev, oracle, ft):
    """One stream, no parallel branches: the entry is a pure launch sequence (no allocation, no synchronisation)."""
    wr, tps = P.WarmRainParams2M(ft, True), P.ThermodynamicsParameters(ft)
    n = 1000
    cols = [c[:n].contiguous() for c in _dev_cols(JC.reference(True)[0], ft, dev)]
    out = (torch.empty((4, 6, n), dtype=DT[ft], device=dev), torch.empty((4, n), dtype=DT[ft], device=dev))
    call = lambda: cmx.warm_rain_jacobian_2m(wr, tps, *cols, with_tendencies=True, out=out)  # noqa: E731
    call()
    torch.cuda.synchronize()
    eager = [o.clone() for o in out]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for o in out:
        o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert _eq(out[0], eager[0]) and _eq(out[1], eager[1])
    # new state in the captured columns: the replay follows it and equals an eager call on the same memory
    for c in cols:
        c.copy_(c.flip(0))
    g.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in out]
    assert not _eq(replayed[0], eager[0])
    call()
    torch.cuda.synchronize()
    assert _eq(out[0], replayed[0]) and _eq(out[1], replayed[1])
