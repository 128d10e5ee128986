"""SB2006 precipitation susceptibilities (src/PrecipitationSusceptibility.jl) on the device (-m gpu), through the C ABI
(cmx_sb2006_precip_susceptibility_*) and cmx.precipitation_susceptibility, in both float types.  The float64 yardstick is the NumPy restatement
tests/precip_susceptibility_ref.py at the float type's gates (pinned by the fixture, the reference test's own formulas and log-differences of the
oracle's rates in tests/test_precip_susceptibility_host.py).  Bound: |x − ref| ≤ rtol·max(|ref|, 1), rtol = 1e-6 (Float64) / 1e-3 (Float32), at every
ungated state; only the autoconversion outputs of states with |x̄_c/x_star − 1| < 1e-5 are set aside (share ≤ 1e-3)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import precip_susceptibility_ref as R
from cmx import _lib
from cmx import parameters as P
from cmx._cols import _fam_of, _ptr
from test_precip_susceptibility_host import KATS, NEAR_CAP, OUTS, RTOL, compare, draw, group_shares, near_clip

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
API_FIELD = {"d_ln_q_lcl": "d_ln_pp_d_ln_q_lcl", "d_ln_q_rai": "d_ln_pp_d_ln_q_rai", "d_ln_N_lcl": "d_ln_pp_d_ln_N_lcl"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(x, ft, dev):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=DT[ft], device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def abi(ft, cols, want=OUTS, outs=None, sb=None):
    """the C entry on the current stream; `outs`: name → preallocated column (default: fresh ones filled with −7)"""
    sb = sb or P.SB2006(ft)
    ref = cols[0]
    if outs is None:
        outs = {k: torch.full_like(ref, -7.0) for k in want}
    au, ac = any(k.startswith("acnv") for k in want), any(k.startswith("accr") for k in want)
    _lib.call("cmx_sb2006_precip_susceptibility", _fam_of(ref), ref.device, C.byref(sb.acnv) if au else None, C.byref(sb.accr) if ac else None,
              ref.numel(), *[_ptr(c) for c in cols], *[_ptr(outs.get(k)) for k in OUTS])
    return outs


def api(ft, cols, fused=True):
    """the Python API, as the same name → column dict"""
    import cmx
    sb = P.SB2006(ft)
    if fused:
        r = cmx.precipitation_susceptibilities(sb, *cols)
        au, ac = r.autoconversion, r.accretion
    else:
        au, ac = cmx.precipitation_susceptibility_autoconversion(sb, *cols), cmx.precipitation_susceptibility_accretion(sb, *cols)
    out = {}
    for proc, r in (("acnv", au), ("accr", ac)):
        for f, name in API_FIELD.items():
            out[f"{proc}_{f}"] = getattr(r, name)
        assert r.d_ln_pp_d_ln_N_rai.shape == cols[0].shape and r.d_ln_pp_d_ln_N_rai.stride() == (0,) and not bool(r.d_ln_pp_d_ln_N_rai.any())
    return out


# ---- known answers and parity -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_known_answers(dev, ft):
    s = KATS["state"]
    cols = [_t([s[k]] * 5, ft, dev) for k in ("q_lcl", "q_rai", "rho", "N_lcl")]
    tol = KATS["rtol"] if ft == "f64" else RTOL[ft]           # the fixture's own rtol (the reference test's ≈); Float32 at the project's bound
    for got in (abi(ft, cols), api(ft, cols), api(ft, cols, fused=False)):
        for proc, name in (("acnv", "autoconversion"), ("accr", "accretion")):
            for f in R.FIELDS:
                e = KATS[name]["d_ln_pp_" + f]["expected"]
                g = _np(got[f"{proc}_{f}"])
                assert (np.abs(g - e) <= tol * max(abs(e), 1)).all(), (proc, f, g, e)
        assert bool((got["acnv_d_ln_N_lcl"] == -2).all()) and bool((got["accr_d_ln_N_lcl"] == 0).all())      # the literal −2, exactly


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_random_draw_parity(dev, ft):
    """seed 1234, 200 003 states.  NaN where the restatement has NaN and nowhere else; the bound at every other state."""
    x = draw(ft)
    assert x[0].size >= 200_000 and near_clip(x).mean() <= NEAR_CAP
    shares = group_shares(x, ft)
    print(f"\n[precip susceptibility draw] {ft}: {shares}")
    assert all(v >= 0.01 for v in shares.values()), shares
    cols = [_t(a, ft, dev) for a in x]
    got_abi = abi(ft, cols)
    compare({k: _np(v) for k, v in got_abi.items()}, x, ft, "device, C ABI")
    for fused in (True, False):
        got = api(ft, cols, fused)
        compare({k: _np(v) for k, v in got.items()}, x, ft, "device, Python API")
        for k in OUTS:                                            # one kernel: the separate calls give the fused call's bits
            assert torch.equal(_bits(got[k]), _bits(got_abi[k])), (fused, k)


# ---- semantics ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_negative_inputs_give_the_bits_of_their_absolute_values(dev, ft):
    cols = [_t(a, ft, dev) for a in draw(ft, 50_001, 5)]
    full = abi(ft, cols)
    for other in ([c.abs() for c in cols], [-c.abs() for c in cols], [cols[0], -cols[1], cols[2], cols[3]], [cols[0], cols[1], -cols[2], -cols[3]]):
        got = abi(ft, other)
        for k in OUTS:
            assert torch.equal(_bits(got[k]), _bits(full[k])), k


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_a_nan_in_any_one_input_gives_nan_outputs(dev, ft):
    base = draw(ft, 4_099, 9)
    full = abi(ft, [_t(a, ft, dev) for a in base])
    for j in range(4):
        cols = [_t(a, ft, dev) for a in base]
        cols[j][::3] = float("nan")
        got = abi(ft, cols)
        rest = torch.ones(cols[0].numel(), dtype=torch.bool, device=dev)
        rest[::3] = False
        for k in OUTS:
            assert bool(torch.isnan(got[k][::3]).all()), (j, k)
            assert torch.equal(_bits(got[k][rest]), _bits(full[k][rest])), (j, k)
    cols = [_t(a, ft, dev) for a in base]
    cols[2][::2] = 0.0                                            # ρ = 0
    got = abi(ft, cols)
    assert all(bool(torch.isnan(got[k][::2]).all()) for k in OUTS)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_every_null_output_subset_is_bit_identical(dev, ft):
    cols = [_t(a, ft, dev) for a in draw(ft, 100_003, 13)]
    full = abi(ft, cols)
    for r in range(1, 6):
        for want in itertools.combinations(OUTS, r):
            got = abi(ft, cols, want=want)
            assert set(got) == set(want)
            for k in want:
                assert torch.equal(_bits(got[k]), _bits(full[k])), (want, k)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_bad_arguments_are_rejected(dev, ft):
    import cmx
    from cmx import _abi
    sb = P.SB2006(ft)
    cols = [_t(a, ft, dev) for a in draw(ft, 1_000, 3)]
    with pytest.raises(cmx.CmxStatusError) as e:
        abi(ft, cols, want=())                                    # no output requested
    assert e.value.status == _abi.CMX_ERR_BAD_ARG
    fn = getattr(_lib.lib(), f"cmx_sb2006_precip_susceptibility_{ft}")
    out = torch.empty_like(cols[0])
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = [_ptr(c) for c in cols]
    nul = [None] * 5
    assert fn(None, C.byref(sb.accr), 1000, *p, _ptr(out), *nul, s) == _abi.CMX_ERR_BAD_ARG            # acnv output without acnv
    assert fn(C.byref(sb.acnv), None, 1000, *p, *nul, _ptr(out), s) == _abi.CMX_ERR_BAD_ARG            # accr output without accr
    assert fn(C.byref(sb.acnv), C.byref(sb.accr), -1, *p, _ptr(out), *nul, s) == _abi.CMX_ERR_BAD_ARG
    assert fn(C.byref(sb.acnv), C.byref(sb.accr), 1000, p[0], None, p[2], p[3], _ptr(out), *nul, s) == _abi.CMX_ERR_BAD_ARG
    assert fn(C.byref(sb.acnv), C.byref(sb.accr), 0, *p, _ptr(out), *nul, s) == _abi.CMX_OK
    other = "f64" if ft == "f32" else "f32"
    with pytest.raises(TypeError):
        cmx.precipitation_susceptibilities(P.SB2006(other), *cols)                                      # the scheme of the other float type
    with pytest.raises(ValueError):
        cmx.precipitation_susceptibilities(sb, cols[0], cols[1][:-1], cols[2], cols[3])                 # shapes differ
    with pytest.raises(ValueError):
        cmx.precipitation_susceptibility_accretion(sb, cols[0], cols[1], cols[2].to(DT[other]), cols[3])


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_misaligned_views_and_odd_counts_are_bit_identical(dev, ft):
    n = 50_001
    cols = [_t(a, ft, dev) for a in draw(ft, n + 8, 17)]
    full = abi(ft, cols)
    for lo in (1, 2, 3):
        for m in (n, n - 1, 7, 1):
            got = abi(ft, [c[lo:lo + m] for c in cols])
            for k in OUTS:
                assert torch.equal(_bits(got[k]), _bits(full[k][lo:lo + m])), (lo, m, k)
    # mixed offsets between the columns, and misaligned outputs: equal to the call on aligned copies
    mixed = [cols[0][1:1 + n], cols[1][0:n], cols[2][3:3 + n], cols[3][2:2 + n]]
    ref = abi(ft, [c.clone() for c in mixed])
    back = {k: torch.full((n + 8,), -7.0, dtype=DT[ft], device=dev) for k in OUTS}
    got = abi(ft, mixed, outs={k: back[k][1 + i % 3:1 + i % 3 + n] for i, k in enumerate(OUTS)})
    for k in OUTS:
        assert torch.equal(_bits(got[k]), _bits(ref[k])), k
    for i, k in enumerate(OUTS):                                    # nothing written outside the views
        o = 1 + i % 3
        assert bool((back[k][:o] == -7).all()) and bool((back[k][o + n:] == -7).all()), k


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_captured_call_replays_bit_identically(dev, ft):
    n = 65_536 + 3
    cols = [_t(a, ft, dev) for a in draw(ft, n, 19)]
    outs = {k: torch.full_like(cols[0], -7.0) for k in OUTS}
    abi(ft, cols, outs=outs)
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                       # the entry launches on the caller's (capturing) stream
        abi(ft, cols, outs=outs)
    for v in outs.values():
        v.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    for k in OUTS:
        assert torch.equal(_bits(outs[k]), _bits(eager[k])), k
    for c in cols:                                                  # new state in the captured columns: the replay follows it
        c.copy_(c.flip(0))
    g.replay()
    torch.cuda.synchronize()
    again = abi(ft, cols)
    for k in OUTS:
        assert torch.equal(_bits(outs[k]), _bits(again[k])), k
    assert not torch.equal(_bits(outs["acnv_d_ln_q_rai"]), _bits(eager["acnv_d_ln_q_rai"]))
