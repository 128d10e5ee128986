"""The sub-stepped implicit average on the device (cmx_sb2006_warm_rain_implicit_average_*, cmx_mp1m_implicit_average_*; cmx.warm_rain_implicit_average_2m,
cmx.implicit_average_1m): the fused call against THE RECIPE — the definition of include/cmx.h §19 in torch over the device's own implicit entry
(tests/implicit_average_cases.py) — bit for bit, for every scheme, float type and option case; the non-negativity the limiter gives; subset independence
through the raw ABI, the NaN rule, misaligned columns, a 3-D shape, `out=` and in place, n = 0, graph capture.

The device average against the host build of the same float type is counted and printed, not asserted: the device Jacobian's columns are not the host
build's bit for bit (tests/test_implicit_gpu.py).  No shape is larger than 4097 points."""
import ctypes as C

import numpy as np
import pytest
import torch

import implicit_average_cases as AC
import jacobian_products_cases as PC
from jacobian_host_build import host_fixture
import cmx
from cmx import _abi, _lib
from cmx import parameters as P

pytestmark = pytest.mark.gpu
host = host_fixture("implicit_average_host")
DT = {"f32": torch.float32, "f64": torch.float64}
FTS = ["f64", "f32"]
SIZES = (1, 255, 257, 4097)
API = {"sb2006": dict(average=cmx.warm_rain_implicit_average_2m, implicit=cmx.warm_rain_implicit_tendencies_2m, stem="cmx_sb2006_warm_rain"),
       "mp1m": dict(average=cmx.implicit_average_1m, implicit=cmx.implicit_tendencies_1m, stem="cmx_mp1m")}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _eq(a, b):
    """Same bits, NaN = NaN."""
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


def _setup(oracle, name, case, ft, dev, n=SIZES[-1]):
    """(api, scheme, mp, tps, host columns, device columns): the LAST n states of the scheme's set — the pinned points, one of them without rain, included."""
    scheme, api = PC.SCHEMES[name], API[name]
    host_cols = [np.array(c[-n:]) for c in AC.STATES[name](oracle)]
    cols = [torch.from_numpy(c).to(DT[ft]).to(dev) for c in host_cols]
    return api, scheme, scheme.params(ft, case), P.ThermodynamicsParameters(ft), host_cols, cols


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_fused_equals_the_device_recipe_bit_for_bit(dev, host, oracle, name, case, ft):
    """nsub ∈ {1, 2, 5}, Δt ∈ {1, 30, 300}, with and without the limiter, on 4097 states: every bit of the fused call is the recipe's.  A shorter call equals
    the head of the longest.  Against the host build: counted and printed."""
    api, scheme, mp, tps, host_cols, cols = _setup(oracle, name, case, ft, dev)
    n = SIZES[-1]
    head = PC.head(scheme, ft, case)[1]
    full = {}
    for dt in AC.DTS:
        for nsub in AC.NSUBS:
            for nonneg in (True, False):
                got = api["average"](mp, tps, *cols, dt, nsub, nonneg)
                want = AC.device_recipe(api["implicit"], name, ft, mp, tps, cols, dt, nsub, nonneg)
                assert got.shape == (4, n)
                assert _eq(got, want), (dt, nsub, nonneg, int(((got != want) & ~(torch.isnan(got) & torch.isnan(want))).sum()))
                full[dt, nsub, nonneg] = got
    for m in SIZES[:-1]:
        short = [c[:m].contiguous() for c in cols]
        for key in ((30.0, 2, True), (300.0, 5, False)):
            assert _eq(api["average"](mp, tps, *short, *key), full[key][:, :m]), (m, key)
    for key in ((30.0, 1, True), (30.0, 5, True), (300.0, 5, False)):
        a = full[key].cpu().numpy()
        a_host, rc = AC.host_average(host, name, ft, head, key[0], key[1], host_cols, key[2])
        assert rc == _abi.CMX_OK
        differ = int((a.view(np.uint8) != a_host.view(np.uint8)).reshape(4, n, -1).any(axis=-1).sum())
        with np.errstate(all="ignore"):
            rel = np.abs(a.astype(np.float64) - a_host) / np.maximum(np.abs(a_host.astype(np.float64)), 1e-300)
        print(f"{name} {case} {ft} dt={key[0]} nsub={key[1]} nonnegative={key[2]}: {differ} of {a.size} elements differ in bits from the host build, "
              f"median relative difference {np.nanmedian(rel):.3g}")


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_no_species_ends_negative_with_the_limiter_and_many_do_without(dev, oracle, name, ft):
    """The property of tests/test_implicit_average_host.py on the device: with the limiter average·Δt ≥ −s0·(1 + 4 eps) for every species with s0 ≥ 0 and
    every output finite; without it, at Δt = 30 s and nsub = 1, at least 5 % of the states violate it."""
    api, scheme, mp, tps, host_cols, cols = _setup(oracle, name, AC.DEFAULT[name], ft, dev)
    for dt in AC.DTS:
        for nsub in AC.NSUBS:
            avg = api["average"](mp, tps, *cols, dt, nsub, True).cpu().numpy()
            assert np.isfinite(avg).all(), (dt, nsub)
            assert AC.negative_share(ft, avg, host_cols, dt) == 0.0, (dt, nsub)
    share = AC.negative_share(ft, api["average"](mp, tps, *cols, 30.0, 1, False).cpu().numpy(), host_cols, 30.0)
    print(f"{name} {ft}: without the limiter {share:.1%} of the states end with a negative species (dt = 30 s, nsub = 1)")
    assert share >= 0.05, share


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_a_requested_subset_equals_the_full_call(dev, oracle, name, case, ft):
    """Through the raw ABI: any member of `average` may be NULL; a column that is written does not depend on which others are, bit for bit, and a buffer that
    was not requested keeps its sentinel."""
    api, scheme, mp, tps, _, cols = _setup(oracle, name, case, ft, dev, 257)
    fam = _abi.F32 if ft == "f32" else _abi.F64
    flags = scheme.flags(mp, case)
    tab = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    state = [C.c_void_p(c.data_ptr()) for c in cols]
    full = api["average"](mp, tps, *cols, 30.0, 2, True)
    rng = np.random.default_rng(3)
    for trial in range(4):
        want = rng.random(4) < 0.5
        want[trial] = True
        got = torch.full((4, 257), -7.0, dtype=DT[ft], device=dev)
        _lib.call(api["stem"] + "_implicit_average", fam, dev, C.byref(mp.c), C.byref(tps), flags, 257, *state, 30.0, 2, _abi.CMX_STEP_NONNEGATIVE,
                  tab([got[q] if want[q] else None for q in range(4)]))
        torch.cuda.synchronize()
        for q in range(4):
            assert _eq(got[q], full[q]) if want[q] else bool((got[q] == -7.0).all()), (trial, q)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_a_nan_poisons_every_output_of_its_point_only(dev, oracle, name, case, ft):
    """One point of 130, every state column; the 1-moment Float64 entry also for ρ ≤ 0."""
    api, scheme, mp, tps, _, cols = _setup(oracle, name, case, ft, dev, 130)
    clean = api["average"](mp, tps, *cols, 30.0, 2, True)
    others = torch.arange(130, device=dev) != 77
    for j, v in [(j, float("nan")) for j in range(7)] + ([(0, 0.0), (0, -1.0)] if (name, ft) == ("mp1m", "f64") else []):
        bad = [c.clone() for c in cols]
        bad[j][77] = v
        a = api["average"](mp, tps, *bad, 30.0, 2, True)
        assert bool(torch.isnan(a[:, 77]).all()) and _eq(a[:, others], clean[:, others]), (j, v)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_misaligned_columns_3d_shape_out_and_in_place(dev, oracle, name, ft):
    api, scheme, mp, tps, _, base = _setup(oracle, name, AC.DEFAULT[name], ft, dev, 1000)
    ref = api["average"](mp, tps, *base, 30.0, 2, True)
    # every column offset by one element from its allocation: no column starts on a 16-byte boundary; guard values on both sides
    n = 257
    cols = [torch.cat([c[:1], c[:n]])[1:] for c in base]
    buf = torch.full((1 + 4 * n + 1,), -7.0, dtype=DT[ft], device=dev)
    o = buf[1:-1].view(4, n)
    assert all(c.data_ptr() % 16 != 0 for c in cols) and o.data_ptr() % 16 != 0
    a = api["average"](mp, tps, *cols, 30.0, 2, True, out=o)
    assert a.data_ptr() == o.data_ptr() and _eq(o, ref[:, :n])
    assert float(buf[0]) == float(buf[-1]) == -7.0      # nothing written outside the columns
    # a 3-D column shape
    cube = [c[:990].reshape(5, 18, 11).contiguous() for c in base]
    a = api["average"](mp, tps, *cube, 30.0, 2, True)
    assert a.shape == (4, 5, 18, 11) and _eq(a.reshape(4, 990), ref[:, :990])
    # the wrapper's argument checks
    for bad in (dict(dt=-1.0), dict(dt=0.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(nsub=0), dict(nsub=65), dict(nsub=1.5),
                dict(out=torch.empty((3, 1000), dtype=DT[ft], device=dev))) + ((dict(dt=2e-38, nsub=64),) if ft == "f32" else ()):
        kw = dict(dt=30.0, nsub=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            api["average"](mp, tps, *base, kw.pop("dt"), **kw)
    # in place: the average written over the four species columns (a lane reads everything it needs before it writes)
    state = torch.stack(base)
    a = api["average"](mp, tps, *state, 30.0, 2, True, out=state[3:7])
    assert a.data_ptr() == state[3].data_ptr() and _eq(state[3:7], ref) and all(_eq(state[j], base[j]) for j in range(3))
    # n = 0 returns without touching memory
    guard = torch.full((8,), -7.0, dtype=DT[ft], device=dev)
    a = api["average"](mp, tps, *[guard[4:4] for _ in range(7)], 30.0, 2, True, out=guard[4:4].view(4, 0))
    torch.cuda.synchronize()
    assert a.numel() == 0 and bool((guard == -7.0).all())


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_a_captured_call_replays_bit_identically(dev, oracle, name, ft):
    """One call on one stream: the entry is a pure launch sequence (no allocation, no synchronisation)."""
    api, scheme, mp, tps, _, cols = _setup(oracle, name, AC.DEFAULT[name], ft, dev, 1000)
    out = torch.empty((4, 1000), dtype=DT[ft], device=dev)

    def call():
        api["average"](mp, tps, *cols, 30.0, 2, True, out=out)
    call()
    torch.cuda.synchronize()
    eager = out.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert _eq(out, eager)
    # new state in the captured columns: the replay follows it and equals an eager call on the same memory
    for c in cols:
        c.copy_(c.flip(0))
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    assert not _eq(replayed, eager)
    call()
    torch.cuda.synchronize()
    assert _eq(out, replayed)
