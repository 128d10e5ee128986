"""The sub-stepped implicit average (include/cmx.h §19) without a GPU: the driver's implicit_average_point (csrc/cmx_jacobian.hpp) in the host build
tests/native/implicit_average_host.cpp against THE RECIPE — the definition of §19 in NumPy over the host build of the implicit entry
(tests/implicit_average_cases.py) — bit for bit; the non-negativity the limiter gives and the plain step does not; first order in Δt/nsub; a linear toy scheme
against its closed form; the NaN rule, subset independence; and the argument statuses of the device entries.

Measured with this host build (Float64, default options, Δt = 30 s, nsub = 1, the states of tests/implicit_cases.py): without the limiter a species that
started ≥ 0 ends negative at 17 % of the SB2006 and 58 % of the 1-moment states; with it at none, every output finite.  Median error ratios when nsub doubles
(reference: the recipe at nsub = 1024): SB2006 e(8)/e(16) = 1.98, e(16)/e(32) = 2.01; 1-moment 1.99, 2.02.  The toy scheme uses at most 0.09 of its bound."""
import ctypes as C
import functools

import numpy as np
import pytest

import implicit_average_cases as AC
import implicit_cases as IC
from jacobian_host_build import NPT, _same_bits, host_fixture
from cmx import _abi, _lib
from cmx import parameters as P

host = host_fixture("implicit_average_host")
implicit_host = host_fixture("implicit_host")
FTS = ["f64", "f32"]


# ---- 1. the fused host build is the recipe, in every bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", AC.CASES)
def test_fused_equals_the_recipe_bit_for_bit(host, implicit_host, oracle, name, case, ft):
    """Both schemes, both float types, every option case, nsub ∈ {1, 2, 5}, Δt ∈ {1, 30, 300}, with and without the limiter, on the full state sets."""
    _, head = AC.head(name, ft, case)
    cols = AC.STATES[name](oracle)
    for dt in AC.DTS:
        for nsub in AC.NSUBS:
            for nonneg in (True, False):
                got, rc = AC.host_average(host, name, ft, head, dt, nsub, cols, nonneg)
                assert rc == _abi.CMX_OK
                want = AC.host_recipe(implicit_host, name, ft, head, dt, nsub, cols, nonneg)
                assert _same_bits(got, want), (dt, nsub, nonneg, int((got.view(np.uint8) != want.view(np.uint8)).reshape(got.shape + (-1,)).any(axis=-1).sum()))


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_the_average_does_not_depend_on_the_tangent_width(host, oracle, name, ft):
    _, head = AC.head(name, ft, AC.DEFAULT[name])
    cols = [c[-513:] for c in AC.STATES[name](oracle)]
    full, rc = AC.host_average(host, name, ft, head, 30.0, 2, cols, k=1)
    assert rc == _abi.CMX_OK
    for k in (0, 2, 4):
        got, rc = AC.host_average(host, name, ft, head, 30.0, 2, cols, k=k)
        assert rc == _abi.CMX_OK and _same_bits(got, full), k


# ---- 2. non-negativity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_no_species_ends_negative_with_the_limiter_and_many_do_without(host, oracle, name, ft):
    """With CMX_STEP_NONNEGATIVE, for every species with s0 ≥ 0: average·Δt ≥ −s0·(1 + 4 eps) (two roundings of the difference and the product each side of
    s_end ≥ 0), and every output is finite — at every Δt and nsub.  Without it, at Δt = 30 s and nsub = 1, at least 5 % of the states violate it (measured:
    module docstring): the assertion has teeth."""
    _, head = AC.head(name, ft, AC.DEFAULT[name])
    cols = AC.STATES[name](oracle)
    for dt in AC.DTS:
        for nsub in AC.NSUBS:
            avg, rc = AC.host_average(host, name, ft, head, dt, nsub, cols, True)
            assert rc == _abi.CMX_OK and np.isfinite(avg).all(), (dt, nsub)
            assert AC.negative_share(ft, avg, cols, dt) == 0.0, (dt, nsub)
    avg, rc = AC.host_average(host, name, ft, head, 30.0, 1, cols, False)
    share = AC.negative_share(ft, avg, cols, 30.0)
    print(f"{name} {ft}: without the limiter {share:.1%} of the states end with a negative species (dt = 30 s, nsub = 1)")
    assert rc == _abi.CMX_OK and share >= 0.05, share


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_a_negative_species_never_ends_below_where_it_started(host, oracle, name, ft):
    _, head = AC.head(name, ft, AC.DEFAULT[name])
    cols = [c[-1025:].copy() for c in AC.STATES[name](oracle)]
    for j in (3, 5):
        cols[j][::3] = -1e-7 * (1.0 + np.arange(cols[j][::3].size) % 5)
    for nsub in AC.NSUBS:
        avg, rc = AC.host_average(host, name, ft, head, 30.0, nsub, cols, True)
        assert rc == _abi.CMX_OK and np.isfinite(avg).all()
        s0 = np.stack([np.asarray(c, dtype=NPT[ft]).astype(np.float64) for c in cols[3:7]])
        step = avg.astype(np.float64) * 30.0
        assert (step[s0 < 0] >= -np.abs(s0[s0 < 0]) * 4.0 * IC.EPS[ft]).all(), nsub      # s_end ≥ s0 where s0 < 0
        assert AC.negative_share(ft, avg, cols, 30.0) == 0.0, nsub


# ---- 3. first order ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_1024(name):
    import oracle_binding as oracle
    from jacobian_host_build import _build
    _, head = AC.head(name, "f64", AC.DEFAULT[name])
    return AC.host_recipe(_build("implicit_host"), name, "f64", head, 30.0, 1024, AC.STATES[name](oracle), True)


@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_first_order_in_the_substep(host, oracle, name):
    """Float64, default options, limiter on, Δt = 30 s.  Reference: the NumPy recipe at nsub = 1024.  e(nsub) = max_j |a_j − ref_j| / (|ref_j| + 1e-12·max over
    points of |ref_j|); the medians over the states of e(8)/e(16) and e(16)/e(32) lie in [1.7, 2.3] (theory: 2)."""
    _, head = AC.head(name, "f64", AC.DEFAULT[name])
    cols = AC.STATES[name](oracle)
    ref = _reference_1024(name)
    floor = 1e-12 * np.abs(ref).max(axis=1, keepdims=True)
    e = {}
    for nsub in (8, 16, 32):
        avg, rc = AC.host_average(host, name, "f64", head, 30.0, nsub, cols, True)
        assert rc == _abi.CMX_OK
        e[nsub] = (np.abs(avg - ref) / (np.abs(ref) + floor)).max(axis=0)
    for a, b in ((8, 16), (16, 32)):
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = e[a] / e[b]
        med = float(np.median(ratio[~np.isnan(ratio)]))
        print(f"{name}: median e({a})/e({b}) = {med:.3f} over {int((~np.isnan(ratio)).sum())} states")
        assert 1.7 <= med <= 2.3, (a, b, med)


# ---- 4. the linear toy scheme ------------------------------------------------------------------------------------------------------------------------
G = -np.array([[4.0, 0.5, 0.25, 1.0], [0.75, 3.0, 0.5, 0.125], [1.0, 0.25, 5.0, 0.5], [0.5, 1.0, 0.75, 2.0]]) / 64.0      # tests/test_implicit_host.py


@pytest.mark.parametrize("ft", FTS)
def test_toy_matches_the_closed_form(host, ft):
    """f = M s, no temperature, no limiter: every substep is s ← (I − hM)⁻¹ s, so the average is ((I − hM)⁻ⁿˢᵘᵇ − I) s0 / Δt, formed here in Float64.
    Bound: a substep's r has a forward error of a few eps·κ∞(I − hM) relative to the state (tests/test_implicit_host.py: (8 κ∞ + 4) eps per solve), nsub ≤ 5 of
    them add up and the last subtraction and the division by Δt act on values of the size of the state, so
        max_j |average_j − ref_j| ≤ 64 eps κ∞(I − hM) · max_j |s0_j| / Δt."""
    rng = np.random.default_rng(3)
    s0 = [10.0 ** rng.uniform(-4.0, -2.0, 257) for _ in range(4)]
    cols = [np.ones(257)] + s0
    M = np.asarray(G, dtype=NPT[ft]).astype(np.float64)
    s64 = np.stack([np.asarray(c, dtype=NPT[ft]).astype(np.float64) for c in s0], axis=1)
    for dt in AC.DTS:
        for nsub in AC.NSUBS:
            avg, rc = AC.host_average(host, "toy", ft, IC.head_toy(ft, G), dt, nsub, cols, False)
            assert rc == _abi.CMX_OK and np.isfinite(avg).all()
            h = float(NPT[ft](dt) / NPT[ft](nsub))
            A = np.eye(4) - h * M
            P_ = np.linalg.matrix_power(np.linalg.inv(A), nsub)
            ref = (s64 @ (P_ - np.eye(4)).T) / float(NPT[ft](dt))
            kappa = np.abs(A).sum(axis=1).max() * np.abs(np.linalg.inv(A)).sum(axis=1).max()
            err = np.abs(avg.T.astype(np.float64) - ref).max(axis=1)
            lim = 64.0 * IC.EPS[ft] * kappa * np.abs(s64).max(axis=1) / dt
            print(f"toy {ft} dt={dt} nsub={nsub}: worst error / bound {(err / lim).max():.3g}, κ∞ = {kappa:.3g}")
            assert (err <= lim).all(), (dt, nsub, (err / lim).max())


# ---- 5. the device entries' argument statuses (no launch is reached) --------------------------------------------------------------------------------
def test_argument_statuses_without_gpu():
    lib = _lib.lib()
    BAD, OK, UNSUPPORTED = _abi.CMX_ERR_BAD_ARG, _abi.CMX_OK, _abi.CMX_ERR_UNSUPPORTED
    cols, table = [C.c_void_p(4096)] * 7, (C.c_void_p * 4)(*[4096 + 64 * k for k in range(4)])
    empty = (C.c_void_p * 4)()
    huge = 16 * 0x7fffffff + 1
    NN = _abi.CMX_STEP_NONNEGATIVE
    for sfx in ("f32", "f64"):
        tps = P.ThermodynamicsParameters(sfx)
        wr, mp = P.WarmRainParams2M(sfx), P.Microphysics1MParams(sfx)
        for f, p, flags in ((getattr(lib, f"cmx_sb2006_warm_rain_implicit_average_{sfx}"), wr.c, 1), (getattr(lib, f"cmx_mp1m_implicit_average_{sfx}"), mp.c, mp.flags)):
            call = lambda *a: f(C.byref(p), C.byref(tps), flags, *a)      # noqa: E731
            assert f(None, C.byref(tps), flags, 10, *cols, 30.0, 1, NN, table, None) == BAD
            assert f(C.byref(p), None, flags, 10, *cols, 30.0, 1, NN, table, None) == BAD
            assert call(-1, *cols, 30.0, 1, NN, table, None) == BAD
            assert call(10, *([None] * 7), 30.0, 1, NN, table, None) == BAD                # NULL columns
            assert call(10, *cols[:6], None, 30.0, 1, NN, table, None) == BAD
            assert call(10, *cols, 30.0, 1, NN, None, None) == BAD                         # `average` NULL itself
            assert call(10, *cols, 30.0, 1, NN, empty, None) == BAD                        # no output column at all
            for nsub in (0, 65, -1):
                assert call(10, *cols, 30.0, nsub, NN, table, None) == BAD, nsub
            for dt in (0.0, -1.0, -0.5e-300, float("nan"), float("inf"), float("-inf")):
                assert call(10, *cols, dt, 1, NN, table, None) == BAD, dt
            for bits in (2, 3, 1 << 31):
                assert call(10, *cols, 30.0, 1, bits, table, None) == BAD, bits             # an unknown step flag
            # the order: the count rule and n = 0 come first, as in the implicit entry of the scheme; the step is checked after the columns
            assert call(huge, *cols, -1.0, 0, 2, None, None) == UNSUPPORTED
            assert call(0, *([None] * 7), -1.0, 0, 2, None, None) == OK
            assert call(0, *cols, float("nan"), 65, NN, table, None) == OK
        f1 = getattr(lib, f"cmx_mp1m_implicit_average_{sfx}")
        assert f1(C.byref(mp.c), C.byref(tps), 1 << 17, 0, *cols, 30.0, 1, NN, table, None) == BAD      # the flags come before n = 0 there
        fs = getattr(lib, f"cmx_sb2006_warm_rain_implicit_average_{sfx}")
        assert fs(C.byref(wr.c), C.byref(tps), 4, 0, *cols, 30.0, 1, NN, table, None) == OK               # … and after the columns here
    # a Float32 Δt whose substep h = Δt/nsub is no normal number (2e-38/64 is subnormal), or whose reciprocal overflows; Float64 holds both
    tps, wr, mp = P.ThermodynamicsParameters("f32"), P.WarmRainParams2M("f32"), P.Microphysics1MParams("f32")
    for f, p, flags in ((lib.cmx_sb2006_warm_rain_implicit_average_f32, wr.c, 1), (lib.cmx_mp1m_implicit_average_f32, mp.c, mp.flags)):
        assert f(C.byref(p), C.byref(tps), flags, 10, *cols, 2e-38, 64, NN, table, None) == BAD
        assert f(C.byref(p), C.byref(tps), flags, 10, *cols, 1e-39, 1, NN, table, None) == BAD
        assert f(C.byref(p), C.byref(tps), flags, 10, *cols, 1e39, 1, NN, table, None) == BAD             # FT(dt) = Inf


def test_host_mirror_statuses(host):
    """The host mirrors report what the entries report after the columns."""
    BAD = _abi.CMX_ERR_BAD_ARG
    cols = [np.ones(4) * v for v in (1.0, 280.0, 1e-2, 1e-3, 1e8, 1e-4, 1e3)]
    for ft in FTS:
        _, head = AC.head("sb2006", ft, (True, False))
        assert AC.host_average(host, "sb2006", ft, head, 30.0, 1, cols, no_table=True)[1] == BAD
        assert AC.host_average(host, "sb2006", ft, head, 30.0, 1, cols, null=(0, 1, 2, 3))[1] == BAD
        assert AC.host_average(host, "sb2006", ft, head, 30.0, 0, cols)[1] == BAD
        assert AC.host_average(host, "sb2006", ft, head, 30.0, 65, cols)[1] == BAD
        assert AC.host_average(host, "sb2006", ft, head, 0.0, 1, cols)[1] == BAD
        assert AC.host_average(host, "sb2006", ft, head, 30.0, 1, cols, step_flags=2)[1] == BAD
        assert AC.host_average(host, "sb2006", ft, head, 30.0, 64, cols)[1] == _abi.CMX_OK
    _, head = AC.head("sb2006", "f32", (True, False))
    assert AC.host_average(host, "sb2006", "f32", head, 2e-38, 64, cols)[1] == BAD


# ---- 6. the NaN rule and subset independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_nan_rule_and_subset_independence(host, oracle, name, ft):
    """A NaN in any of the seven inputs of a point gives NaN in all four averages of that point and changes no other point; the 1-moment Float64 entry does
    the same for ρ ≤ 0.  A requested subset equals the same columns of the full call; a column that was not requested keeps its sentinel."""
    _, head = AC.head(name, ft, AC.DEFAULT[name])
    cols = [c[-16:].copy() for c in AC.STATES[name](oracle)]
    clean, rc = AC.host_average(host, name, ft, head, 30.0, 2, cols)
    assert rc == _abi.CMX_OK and np.isfinite(clean).all()
    keep = np.arange(16) != 5
    for j, v in [(j, np.nan) for j in range(7)] + ([(0, 0.0), (0, -1.0)] if (name, ft) == ("mp1m", "f64") else []):
        bad = [c.copy() for c in cols]
        bad[j][5] = v
        avg, _ = AC.host_average(host, name, ft, head, 30.0, 2, bad)
        assert np.isnan(avg[:, 5]).all() and _same_bits(avg[:, keep], clean[:, keep]), (j, v)
    for null in [(0,), (1, 3), (0, 1, 2)]:
        avg, rc = AC.host_average(host, name, ft, head, 30.0, 2, cols, null=null, sentinel=7.0)
        got = [q for q in range(4) if q not in null]
        assert rc == _abi.CMX_OK and _same_bits(avg[got], clean[got]) and (avg[list(null)] == 7.0).all(), null
