"""The 1-moment tendency Jacobian on the device (cmx_mp1m_jacobian_*, cmx.jacobian_1m): the parity assertions of tests/test_mp1m_jacobian_host.py through
the kernel (same states, same finite-difference reference of the Float64 oracle, same bounds, same 1 % condition — tests/jacobian_1m_cases.py — in both of its measures: the per-row one of the reference and the input-scaled one, which resolves the T column; worst
input-scaled value on the device 9.7e-8 in Float64 and 4.9e-4 in Float32, dq_icl_dt × T with the alternative options on the cold set, every other Float32
entry ≤ 4.6e-5), the primal
against cmx.bulk_microphysics_tendencies_1m bit for bit, column selection, the edges of the launch path, the poison rules and graph capture.  No shape is
larger than 4096 points."""
import ctypes as C

import numpy as np
import pytest
import torch

import jacobian_1m_cases as JC
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


def _mixed(ft, dev, n):
    """n states, half from the cold and half from the warm interior set."""
    cold, warm = JC.reference("default", "cold")[0], JC.reference("default", "warm")[0]
    return _dev_cols([np.concatenate([a[:n - n // 2], b[:n // 2]]) for a, b in zip(cold, warm)], ft, dev)


def _tendencies(mp, tps, cols):
    return torch.stack(list(cmx.bulk_microphysics_tendencies_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), mp, tps, *cols)))


# ---- parity -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("case", JC.CASES)
def test_jacobian_matches_central_differences_of_the_oracle(dev, oracle, ft, case):
    """Float64: every row of every kept state inside the reference's own 1e-5 (test/ad_compat_tests.jl:163).  Float32 against the same Float64 reference:
    every row inside 1e-3.  Both in the per-row and, every (row, column), in the input-scaled measure.  "default" runs the compile-time instantiation, "alt" and "exponents" the run-time-flags one."""
    mp, tps = JC.params(ft, case), P.ThermodynamicsParameters(ft)
    for which in JC.SETS:
        cols = _dev_cols(JC.reference(case, which)[0], ft, dev)
        r = cmx.jacobian_1m(mp, tps, *cols)
        assert r.tendencies is None and r.wrt == JC.WRT and r.jac.shape == (4, 6, cols[0].numel()) and r.jac.is_contiguous()
        JC.assert_parity(ft, r.jac.cpu().numpy(), case, which, "device")
    if case == "exponents":          # this set is not mp1m_default_exponents: its tendencies differ from the default set's
        a, b = _tendencies(JC.params(ft, "default"), tps, cols), _tendencies(mp, tps, cols)
        assert bool((a[2:] != b[2:]).any())


# ---- the primal ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("case", JC.CASES)
def test_tendencies_are_bit_identical_to_the_tendencies_entry(dev, oracle, ft, case):
    """with_tendencies=True gives the columns of cmx.bulk_microphysics_tendencies_1m(Instantaneous(), …) on the same tensors, bit for bit, on the interior
    sets and on the broad synthetic set (zeros, negative values, every gate); on the latter every Jacobian entry is finite wherever the four tendencies are."""
    mp, tps = JC.params(ft, case), P.ThermodynamicsParameters(ft)
    sets = [(w, _dev_cols(JC.reference(case, w)[0], ft, dev)) for w in ("cold", "warm")] + [("synthetic", list(synthetic.mp1m_state(4096, dtype=DT[ft], device=dev)))]
    for name, cols in sets:
        want = _tendencies(mp, tps, cols)
        for wrt in (JC.WRT, ("q_sno", "q_tot"), ()):
            r = cmx.jacobian_1m(mp, tps, *cols, wrt=wrt, with_tendencies=True)
            for o in range(4):
                assert _eq(r.tendencies[o], want[o]), (name, wrt, JC.OUT[o])
        r = cmx.jacobian_1m(mp, tps, *cols, with_tendencies=True)
        finite = torch.isfinite(r.tendencies).all(dim=0)
        assert finite.sum() > 0.9 * finite.numel()
        assert bool(torch.isfinite(r.jac[:, :, finite]).all()), name


# ---- column selection ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_a_subset_in_any_order_gives_the_columns_of_the_full_call(dev, oracle, ft):
    mp, tps = JC.params(ft, "default"), P.ThermodynamicsParameters(ft)
    cols = _mixed(ft, dev, 1000)
    full = cmx.jacobian_1m(mp, tps, *cols).jac
    # sizes 1 … 5: below, at and above the tangents per pass (csrc/cmx_mp1m_jacobian.hpp: 2 or 3), multiples of it and not
    for wrt in (("q_rai",), ("q_sno", "T"), ("q_lcl", "T", "q_icl"), ("q_sno", "q_rai", "q_icl", "q_tot"), ("q_rai", "q_tot", "q_icl", "T", "q_lcl"),
                tuple(reversed(JC.WRT))):
        r = cmx.jacobian_1m(mp, tps, *cols, wrt=wrt)
        assert r.jac.shape == (4, len(wrt), 1000) and r.wrt == wrt
        for k, name in enumerate(wrt):
            assert _eq(r.jac[:, k], full[:, JC.WRT.index(name)]), (wrt, name)


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_a_null_member_of_a_row_leaves_the_other_members_unchanged(dev, oracle, ft):
    """The raw ABI: any of the 24 column pointers may be NULL; a column that is written does not depend on which others are, and a buffer that was not
    requested keeps its sentinel."""
    mp, tps = JC.params(ft, "default"), P.ThermodynamicsParameters(ft)
    cols = _mixed(ft, dev, 257)
    full = cmx.jacobian_1m(mp, tps, *cols).jac
    rng = np.random.default_rng(3)
    for trial in range(3):
        wanted = rng.random((4, 6)) < 0.5
        wanted[trial, :] = [True, False, True, False, False, True]
        got = torch.full((4, 6, 257), -7.0, dtype=DT[ft], device=dev)
        ptrs = (C.c_void_p * 24)(*[got[o, j].data_ptr() if wanted[o, j] else None for o in range(4) for j in range(6)])
        _lib.call("cmx_mp1m_jacobian", _abi.F32 if ft == "f32" else _abi.F64, dev, C.byref(mp.c), C.byref(tps), mp.flags, 257,
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
    mp, tps = JC.params(ft, "default"), P.ThermodynamicsParameters(ft)
    base = _mixed(ft, dev, 1000)
    ref = cmx.jacobian_1m(mp, tps, *base, with_tendencies=True)
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        r = cmx.jacobian_1m(mp, tps, *[c[:n].contiguous() for c in base], with_tendencies=True)
        assert _eq(r.jac, ref.jac[:, :, :n]) and _eq(r.tendencies, ref.tendencies[:, :n]), n
        # inputs and outputs as views offset by one element: no column starts on a 16-byte boundary
        shifted = [torch.cat([c[:1], c[:n]])[1:] for c in base]
        jbuf = torch.full((1 + 24 * n + 1,), -7.0, dtype=DT[ft], device=dev)
        tbuf = torch.full((1 + 4 * n + 1,), -7.0, dtype=DT[ft], device=dev)
        out = (jbuf[1:1 + 24 * n].view(4, 6, n), tbuf[1:1 + 4 * n].view(4, n))
        assert all(s.data_ptr() % 16 != 0 for s in shifted) and out[0].data_ptr() % 16 != 0 and out[1].data_ptr() % 16 != 0
        r = cmx.jacobian_1m(mp, tps, *shifted, with_tendencies=True, out=out)
        assert r.jac.data_ptr() == out[0].data_ptr()
        assert _eq(r.jac, ref.jac[:, :, :n]) and _eq(r.tendencies, ref.tendencies[:, :n]), n
        assert float(jbuf[0]) == float(jbuf[-1]) == float(tbuf[0]) == float(tbuf[-1]) == -7.0      # nothing written outside the columns
    # n = 0 returns without touching memory (and before the columns are looked at)
    guard = torch.full((8,), -7.0, dtype=DT[ft], device=dev)
    empty = [guard[4:4] for _ in range(7)]
    r = cmx.jacobian_1m(mp, tps, *empty, with_tendencies=True, out=(guard[4:4].view(4, 6, 0), guard[4:4].view(4, 0)))
    torch.cuda.synchronize()
    assert r.jac.numel() == 0 and bool((guard == -7.0).all())


# ---- the poison rules ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_a_nan_input_poisons_every_output_of_its_point_only(dev, oracle, ft):
    """… and so does ρ ≤ 0 in Float64 (bad_density)."""
    mp, tps = JC.params(ft, "default"), P.ThermodynamicsParameters(ft)
    cols = _mixed(ft, dev, 130)
    clean = cmx.jacobian_1m(mp, tps, *cols, with_tendencies=True)
    others = torch.arange(130, device=dev) != 77
    for j, v in [(j, float("nan")) for j in range(7)] + ([(0, 0.0), (0, -0.5)] if ft == "f64" else []):
        bad = [c.clone() for c in cols]
        bad[j][77] = v
        r = cmx.jacobian_1m(mp, tps, *bad, with_tendencies=True)
        assert bool(torch.isnan(r.jac[:, :, 77]).all()) and bool(torch.isnan(r.tendencies[:, 77]).all()), (j, v)
        assert _eq(r.jac[:, :, others], clean.jac[:, :, others]) and _eq(r.tendencies[:, others], clean.tendencies[:, others]), (j, v)


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_captured_call_replays_bit_identically(dev, oracle, ft):
    """One stream, no parallel branches: the entry is a pure launch sequence (no allocation, no synchronisation)."""
    mp, tps = JC.params(ft, "default"), P.ThermodynamicsParameters(ft)
    n = 1000
    cols = _mixed(ft, dev, n)
    out = (torch.empty((4, 6, n), dtype=DT[ft], device=dev), torch.empty((4, n), dtype=DT[ft], device=dev))
    call = lambda: cmx.jacobian_1m(mp, tps, *cols, with_tendencies=True, out=out)  # noqa: E731
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
