"""The linearly implicit tendency r = (I − Δt J)⁻¹ f on the device (cmx_sb2006_warm_rain_implicit_tendencies_*, cmx_mp1m_implicit_tendencies_*;
cmx.warm_rain_implicit_tendencies_2m, cmx.implicit_tendencies_1m): per scheme, float type and option set — SB2006: LIMITED × integer / general exponents,
1-moment: the default instantiation and the run-time-flags one — the primal against the tendencies entry and r at Δt = 0 bit for bit, r against the host build
(tests/native/implicit_host.cpp), subset independence through the raw ABI, the NaN rule; then the wrapper's `out=` and in-place forms and graph capture.

Device r against the host build of the same float type: the device Jacobian's columns are not the host build's bit for bit (the hardware transcendentals and
the host's libm stand-ins differ, tests/test_sb2006_jacobian_gpu.py), so the differing elements are counted and printed, and what is ASSERTED is the bound of
tests/test_implicit_host.py with the DEVICE Jacobian entry's columns: the componentwise backward error ω of the device r in I − Δt J_device, worst over the
set, at most 4 × that of numpy.linalg.solve on copies of the same system in the float type and never required below 16 eps (tests/implicit_cases.py).
No shape is larger than 4097 points."""
import ctypes as C

import numpy as np
import pytest
import torch

import implicit_cases as IC
import jacobian_products_cases as PC
from jacobian_host_build import host_fixture
import cmx
from cmx import _abi, _lib
from cmx import parameters as P

pytestmark = pytest.mark.gpu
host = host_fixture("implicit_host")
DT = {"f32": torch.float32, "f64": torch.float64}
FTS = ["f64", "f32"]
SIZES = (1, 255, 257, 4097)
# SB2006 (limited, perturbed exponents → the general-exponent instantiation); 1-moment: tests/jacobian_1m_cases.py ("alt": the run-time-flags instantiation)
CASES = [("sb2006", (True, False)), ("sb2006", (False, False)), ("sb2006", (True, True)), ("sb2006", (False, True)), ("mp1m", "default"), ("mp1m", "alt")]


def _tend_2m(mp, tps, cols):
    return torch.stack(list(cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), mp, tps, *cols))[:4])


def _tend_1m(mp, tps, cols):
    return torch.stack(list(cmx.bulk_microphysics_tendencies_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), mp, tps, *cols)))


API = {"sb2006": dict(implicit=cmx.warm_rain_implicit_tendencies_2m, jac=cmx.warm_rain_jacobian_2m, tend=_tend_2m, stem="cmx_sb2006_warm_rain", states=IC.sb2006_states),
       "mp1m": dict(implicit=cmx.implicit_tendencies_1m, jac=cmx.jacobian_1m, tend=_tend_1m, stem="cmx_mp1m", states=IC.mp1m_states)}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _eq(a, b):
    """Same bits, NaN = NaN."""
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


def _setup(oracle, name, case, ft, dev, n=SIZES[-1]):
    """(api, scheme, mp, tps, host columns, device columns): the LAST n states of the scheme's set — the pinned points, one of them without rain, included."""
    scheme, api = PC.SCHEMES[name], API[name]
    host_cols = [np.array(c[-n:]) for c in api["states"](oracle)]
    cols = [torch.from_numpy(c).to(DT[ft]).to(dev) for c in host_cols]
    return api, scheme, scheme.params(ft, case), P.ThermodynamicsParameters(ft), host_cols, cols


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", CASES)
def test_device_r_and_primal(dev, host, oracle, name, case, ft):
    """Every size: `tendencies` bit-identical to the tendencies entry at every Δt, `implicit` bit-identical to it at Δt = 0, a shorter call equal to the
    head of the longest one.  The longest: r against the host build (reported) and the ω bound with the device Jacobian's columns (asserted)."""
    api, scheme, mp, tps, host_cols, cols = _setup(oracle, name, case, ft, dev)
    n = SIZES[-1]
    want = api["tend"](mp, tps, cols)
    full = {}
    for dt in IC.DTS:
        full[dt] = api["implicit"](mp, tps, *cols, dt, with_tendencies=True)
        assert full[dt].implicit.shape == (4, n) and _eq(full[dt].tendencies, want), dt
    assert _eq(full[0.0].implicit, want)
    for m in SIZES[:-1]:
        head = [c[:m].contiguous() for c in cols]
        r = api["implicit"](mp, tps, *head, 30.0, with_tendencies=True)
        assert _eq(r.implicit, full[30.0].implicit[:, :m]) and _eq(r.tendencies, want[:, :m]), m
        assert _eq(api["implicit"](mp, tps, *head, 0.0).implicit, want[:, :m]), m
    jac = api["jac"](mp, tps, *cols, wrt=IC.SPECIES[name], with_tendencies=True)
    J, f = jac.jac.cpu().numpy(), jac.tendencies.cpu().numpy()
    head_ = PC.head(scheme, ft, case)[1]
    for dt in IC.DTS[1:]:
        r = full[dt].implicit.cpu().numpy()
        assert np.isfinite(r).all(), dt
        r_host, _, rc = IC.host_implicit(host, name, ft, head_, dt, host_cols)
        assert rc == _abi.CMX_OK
        differ = int((r.view(np.uint8) != r_host.view(np.uint8)).reshape(4, n, -1).any(axis=-1).sum())
        A, f64 = IC.system(ft, J, f, dt)
        bound, w_lapack = IC.omega_bound(ft, A, f64)
        w = float(IC.omega(A, r.T, f64).max())
        print(f"{name} {case} {ft} dt={dt}: {differ} of {r.size} elements differ in bits from the host build; worst ω device {w:.3g} | LAPACK {w_lapack:.3g} (bound {bound:.3g})")
        assert w <= bound, (dt, w, w_lapack)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", CASES)
def test_a_requested_subset_equals_the_full_call(dev, oracle, name, case, ft):
    """Through the raw ABI: any member of `implicit` and of `tendencies` may be NULL, `tendencies` may be NULL itself; a column that is written does not
    depend on which others are, bit for bit, and a buffer that was not requested keeps its sentinel."""
    api, scheme, mp, tps, _, cols = _setup(oracle, name, case, ft, dev, 257)
    fam = _abi.F32 if ft == "f32" else _abi.F64
    flags = scheme.flags(mp, case)
    tab = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    state = [C.c_void_p(c.data_ptr()) for c in cols]
    full = api["implicit"](mp, tps, *cols, 30.0, with_tendencies=True)
    rng = np.random.default_rng(3)
    for trial in range(4):
        want_r, want_t = rng.random(4) < 0.5, rng.random(4) < 0.5
        want_r[trial] = True
        got_r, got_t = (torch.full((4, 257), -7.0, dtype=DT[ft], device=dev) for _ in range(2))
        _lib.call(api["stem"] + "_implicit_tendencies", fam, dev, C.byref(mp.c), C.byref(tps), flags, 257, *state, 30.0,
                  tab([got_r[q] if want_r[q] else None for q in range(4)]), tab([got_t[q] if want_t[q] else None for q in range(4)]) if trial else None)
        torch.cuda.synchronize()
        for q in range(4):
            assert _eq(got_r[q], full.implicit[q]) if want_r[q] else bool((got_r[q] == -7.0).all()), (trial, q)
            assert _eq(got_t[q], full.tendencies[q]) if (trial and want_t[q]) else bool((got_t[q] == -7.0).all()), (trial, q)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", CASES)
def test_a_nan_poisons_every_output_of_its_point_only(dev, oracle, name, case, ft):
    """One point of 130, every state column; the 1-moment Float64 entry also for ρ ≤ 0."""
    api, scheme, mp, tps, _, cols = _setup(oracle, name, case, ft, dev, 130)
    clean = api["implicit"](mp, tps, *cols, 30.0, with_tendencies=True)
    others = torch.arange(130, device=dev) != 77
    for j, v in [(j, float("nan")) for j in range(7)] + ([(0, 0.0), (0, -1.0)] if (name, ft) == ("mp1m", "f64") else []):
        bad = [c.clone() for c in cols]
        bad[j][77] = v
        r = api["implicit"](mp, tps, *bad, 30.0, with_tendencies=True)
        for a, b in zip(r, clean):
            assert bool(torch.isnan(a[:, 77]).all()) and _eq(a[:, others], b[:, others]), (j, v)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_misaligned_columns_3d_shape_out_and_in_place(dev, oracle, name, ft):
    case = PC.SCHEMES[name].INTERIOR[0]
    api, scheme, mp, tps, _, base = _setup(oracle, name, case, ft, dev, 1000)
    ref = api["implicit"](mp, tps, *base, 30.0, with_tendencies=True)
    # every column offset by one element from its allocation: no column starts on a 16-byte boundary; guard values on both sides
    n = 257
    cols = [torch.cat([c[:1], c[:n]])[1:] for c in base]
    bufs = [torch.full((1 + 4 * n + 1,), -7.0, dtype=DT[ft], device=dev) for _ in range(2)]
    o_r, o_t = [b[1:-1].view(4, n) for b in bufs]
    assert all(c.data_ptr() % 16 != 0 for c in cols) and o_r.data_ptr() % 16 != 0 and o_t.data_ptr() % 16 != 0
    r = api["implicit"](mp, tps, *cols, 30.0, with_tendencies=True, out=(o_r, o_t))
    assert r.implicit.data_ptr() == o_r.data_ptr() and r.tendencies.data_ptr() == o_t.data_ptr()
    assert _eq(o_r, ref.implicit[:, :n]) and _eq(o_t, ref.tendencies[:, :n])
    assert all(float(b[0]) == float(b[-1]) == -7.0 for b in bufs)      # nothing written outside the columns
    # a 3-D column shape
    cube = [c[:990].reshape(5, 18, 11).contiguous() for c in base]
    r = api["implicit"](mp, tps, *cube, 30.0, with_tendencies=True)
    assert r.implicit.shape == (4, 5, 18, 11) and _eq(r.implicit.reshape(4, 990), ref.implicit[:, :990]) and _eq(r.tendencies.reshape(4, 990), ref.tendencies[:, :990])
    # one of the two given in `out=`, the other allocated
    given = torch.empty((4, 1000), dtype=DT[ft], device=dev)
    r = api["implicit"](mp, tps, *base, 30.0, with_tendencies=True, out=(None, given))
    assert r.tendencies.data_ptr() == given.data_ptr() and _eq(given, ref.tendencies) and _eq(r.implicit, ref.implicit)
    with pytest.raises(ValueError):
        api["implicit"](mp, tps, *base, 30.0, out=(None, given))
    with pytest.raises(ValueError):
        api["implicit"](mp, tps, *base, -1.0)
    with pytest.raises(ValueError):
        api["implicit"](mp, tps, *base, float("nan"))
    # in place: r written over the four species columns (a lane reads its point before it writes it)
    state = torch.stack(base)
    r = api["implicit"](mp, tps, *state, 30.0, out=(state[3:7], None))
    assert r.implicit.data_ptr() == state[3].data_ptr() and _eq(state[3:7], ref.implicit) and all(_eq(state[j], base[j]) for j in range(3))
    # n = 0 returns without touching memory
    guard = torch.full((8,), -7.0, dtype=DT[ft], device=dev)
    r = api["implicit"](mp, tps, *[guard[4:4] for _ in range(7)], 30.0, with_tendencies=True, out=(guard[4:4].view(4, 0), guard[4:4].view(4, 0)))
    torch.cuda.synchronize()
    assert r.implicit.numel() == 0 and bool((guard == -7.0).all())


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_a_captured_call_replays_bit_identically(dev, oracle, name, ft):
    """One call on one stream: the entry is a pure launch sequence (no allocation, no synchronisation)."""
    case = PC.SCHEMES[name].INTERIOR[0]
    api, scheme, mp, tps, _, cols = _setup(oracle, name, case, ft, dev, 1000)
    out = [torch.empty((4, 1000), dtype=DT[ft], device=dev) for _ in range(2)]

    def call():
        api["implicit"](mp, tps, *cols, 30.0, with_tendencies=True, out=(out[0], out[1]))
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
    assert all(_eq(o, e) for o, e in zip(out, eager))
    # new state in the captured columns: the replay follows it and equals an eager call on the same memory
    for c in cols:
        c.copy_(c.flip(0))
    g.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in out]
    assert not _eq(replayed[0], eager[0])
    call()
    torch.cuda.synchronize()
    assert all(_eq(o, r) for o, r in zip(out, replayed))
