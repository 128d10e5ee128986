"""The products with the Jacobian without a GPU (include/cmx.h §(16), §(17); csrc/cmx_jacobian.hpp): jvp_point / vjp_point and their argument
tables compiled by g++ for the host (tests/native/derivatives_host.cpp) on SbJac, Mp1mJac and the exact toy scheme.

  * toy scheme: J v and Jᵀḡ equal the exact products, for every tangent width of the VJP;
  * parity through the existing yardstick: J assembled column by column from six J v with unit tangents and row by row from four Jᵀḡ with unit cotangents,
    each through jacobian_cases.assert_parity / jacobian_1m_cases.assert_parity — same states, same finite-difference reference, same bounds (1e-5 / 1e-3 in
    both measures, `float32_bound` for the one exception row), every (case, set), both float types;
  * bit for bit in this build: unit-seed products against the Jacobian's columns and rows, a gradient against the requested subset and the tangent width,
    the primal against the plain instantiation;
  * mixed vectors against the products of the reference at bounds derived from the per-entry bound (tests/jacobian_products_cases.py), and that this check
    can fail: a dropped or swapped tangent column and a negated cotangent are rejected;
  * the NaN rule for a state input, a tangent and a cotangent; the statuses of the entry mirrors.

NULL against zero cotangents: the sum over the given cotangents is plain IEEE, first product then fused multiply-adds, so a cotangent given as zeros adds a
term ±0 where a NULL one adds none.  On the interior set (every tangent finite) that leaves every non-zero gradient value bit-identical and can change only the
SIGN of a gradient that is an exact zero (a sum of zeros: (+0) + (−0) = +0).  The test asserts equality of the values and of the bits of every non-zero one."""
import ctypes as C

import numpy as np
import pytest

import jacobian_products_cases as PC
from jacobian_products_cases import NPT, SCHEME_CASES, SCHEMES, _same_bits, host  # noqa: F401
from cmx import _abi

FTS = ["f64", "f32"]


def _run(host, scheme, ft, case, cols):
    """(head, jvp_of(tangents), vjp_of(cotangents)) of one (scheme, case) on `cols`."""
    mp, hd = PC.head(scheme, ft, case)

    def jvp_of(t):
        y, _, rc = PC.host_jvp(host, scheme.entry, ft, hd, cols, t)
        assert rc >= 0
        return y

    def vjp_of(g, **kw):
        gr, _, rc = PC.host_vjp(host, scheme.entry, ft, hd, cols, g, **kw)
        assert rc >= 0
        return gr
    return (mp, hd), jvp_of, vjp_of


# ---- the toy scheme: exact ------------------------------------------------------------------------------------------------------------------------
def _toy(n=37, seed=2):
    rng = np.random.default_rng(seed)
    x = [rng.integers(-4, 5, n).astype(np.float64) for _ in range(6)]
    rho, a, b, c, d, e = x
    w, z, o = 3.0, np.zeros(n), np.ones(n)
    J = np.array([[rho * b, rho * a, o, z, z], [o, z, d, c, w * o], [b * c, a * c, a * b, e * rho, d * rho]])
    f = np.array([rho * a * b + c, c * d + w * e + a, a * b * c + d * e * rho])
    return w, x, J, f, rng


@pytest.mark.parametrize("ft", FTS)
def test_toy_products_are_exact(host, ft):
    """3 outputs × 5 inputs, small integers: every value, tangent and product is exact in both float types, so == holds; VJP at K = 1 … 5, with a NULL
    tangent / cotangent and with a subset of the gradients."""
    w, x, J, f, rng = _toy()
    hd = (PC.CT[ft](w),)
    v = [rng.integers(-3, 4, x[0].size).astype(np.float64) for _ in range(5)]
    g = [rng.integers(-3, 4, x[0].size).astype(np.float64) for _ in range(3)]
    y, tend, rc = PC.host_jvp(host, "toy", ft, hd, x, v, nout=3)
    assert rc == 0 and np.array_equal(y, np.einsum("ijn,jn->in", J, np.array(v))) and np.array_equal(tend, f)
    y, _, rc = PC.host_jvp(host, "toy", ft, hd, x, [v[0], None, v[2], None, v[4]], nout=3, want=[True, False, True])
    assert rc == 0 and np.array_equal(y[[0, 2]], np.einsum("ijn,jn->in", J[:, [0, 2, 4]], np.array([v[0], v[2], v[4]]))[[0, 2]]) and np.all(y[1] == -7.0)
    for k in (1, 2, 3, 4, 5):
        gr, tend, rc = PC.host_vjp(host, "toy", ft, hd, x, g, nwrt=5, nout=3, k=k)
        assert rc == 0 and np.array_equal(gr, np.einsum("ijn,in->jn", J, np.array(g))) and np.array_equal(tend, f), k
        gr, _, rc = PC.host_vjp(host, "toy", ft, hd, x, [g[0], None, g[2]], nwrt=5, nout=3, k=k, want=[False, True, True, False, True])
        want = np.einsum("ijn,in->jn", J[[0, 2]], np.array([g[0], g[2]]))
        assert rc == 0 and np.array_equal(gr[[1, 2, 4]], want[[1, 2, 4]]) and np.all(gr[[0, 3]] == -7.0), k
        gr, _, rc = PC.host_vjp(host, "toy", ft, hd, x, [None, None, None], nwrt=5, nout=3, k=k)       # no cotangent: zeros
        assert rc == 0 and np.all(gr == 0.0), k


# ---- parity through the existing yardstick --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", SCHEME_CASES)
def test_assembled_jacobians_match_central_differences_of_the_oracle(host, oracle, ft, name, case):
    """J from six unit-tangent J v and J from four unit-cotangent Jᵀḡ, each through the scheme's assert_parity: both measures, the bounds and the exception row
    of tests/jacobian_cases.py / tests/jacobian_1m_cases.py, every set.  Then the mixed-vector bounds on the same sets."""
    scheme = SCHEMES[name]
    for which in scheme.SETS:
        cols, J_ref, kept, _ = scheme.reference(case, which)
        _, jvp_of, vjp_of = _run(host, scheme, ft, case, cols)
        Jc, Jr = PC.assemble(jvp_of, vjp_of, cols[0].size, ft)
        scheme.assert_parity(ft, Jc, case, which, "host J from J v")
        scheme.assert_parity(ft, Jr, case, which, "host J from Jᵀḡ")
        _, v, g, *_ = PC.mixed_vectors(cols, J_ref)
        PC.assert_mixed(ft, jvp_of(list(v)), vjp_of(list(g)), cols, J_ref, kept, f"host {name} {case} {which}")


# ---- bit for bit, in this build -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", SCHEME_CASES)
def test_unit_seed_products_are_the_jacobian_bit_for_bit(host, oracle, ft, name, case):
    """A unit-tangent J v is the Jacobian's column, a unit-cotangent Jᵀḡ its row, and the primal columns of all three are the plain instantiation's."""
    scheme = SCHEMES[name]
    for which in scheme.SETS:
        cols = scheme.reference(case, which)[0]
        (_, hd), jvp_of, vjp_of = _run(host, scheme, ft, case, cols)
        J, tend, rc = PC.host_jacobian(host, scheme.entry, ft, hd, cols)
        assert rc >= 0
        Jc, Jr = PC.assemble(jvp_of, vjp_of, cols[0].size, ft)
        assert _same_bits(Jc, J), (which, "J v")
        assert _same_bits(Jr, J), (which, "Jᵀḡ")
        plain, _ = PC.host_plain(host, scheme.entry, ft, hd, cols)
        one = np.ones(cols[0].size)
        assert _same_bits(tend, plain)
        assert _same_bits(PC.host_jvp(host, scheme.entry, ft, hd, cols, [one] * 6)[1], plain)
        assert _same_bits(PC.host_vjp(host, scheme.entry, ft, hd, cols, [one] * 4)[1], plain)
        assert _same_bits(PC.host_vjp(host, scheme.entry, ft, hd, cols, [None] * 4, want=[False] * 6)[1], plain)      # tendencies alone


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_a_gradient_does_not_depend_on_the_other_requests(host, oracle, ft, name):
    """grad[j] against the requested subset and the tangents per pass, bit for bit; against the other cotangents being NULL or zeros, in value and in the bits
    of every non-zero value (module docstring).  Interior set: every tangent is finite."""
    scheme = SCHEMES[name]
    case, which = scheme.INTERIOR
    cols, J_ref, kept, _ = scheme.reference(case, which)
    cols = [c[:1024] for c in cols]
    _, _, vjp_of = _run(host, scheme, ft, case, cols)
    g = list(PC.mixed_vectors(cols, J_ref[:, :, :1024])[2])
    full = vjp_of(g)
    assert np.isfinite(full).all()
    for k in (1, 2, 3, 6):
        assert _same_bits(vjp_of(g, k=k), full), k
    rng = np.random.default_rng(4)
    for trial in range(6):
        want = list(rng.random(6) < 0.5)
        want[trial] = True
        sub = vjp_of(g, want=want, k=(1, 2, 3)[trial % 3])
        for j in range(6):
            assert _same_bits(sub[j], full[j]) if want[j] else np.all(sub[j] == -7.0), (trial, j)
    zero = np.zeros(1024)
    sign_only = 0
    for given in ([0], [2], [1, 3], [0, 1, 2]):
        a = vjp_of([g[q] if q in given else None for q in range(4)])
        b = vjp_of([g[q] if q in given else zero for q in range(4)])
        assert np.array_equal(a, b), given
        nz = a != 0
        assert _same_bits(a[nz], b[nz]), given
        sign_only += int((np.signbit(a) != np.signbit(b)).sum())
    print(f"{name} {ft}: NULL against zero cotangents — {sign_only} exact zeros differ in sign, every other value in no bit")


# ---- the mixed-vector check can fail --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_a_wrong_product_is_rejected_by_the_mixed_vector_bounds(host, oracle, ft, name):
    """J v with one tangent column dropped, J v with two tangent columns swapped, Jᵀḡ with one cotangent negated: each is rejected, for every column / pair /
    output, while the right products pass."""
    scheme = SCHEMES[name]
    case, which = scheme.INTERIOR
    cols, J_ref, kept, _ = scheme.reference(case, which)
    _, jvp_of, vjp_of = _run(host, scheme, ft, case, cols)
    _, v, g, *_ = PC.mixed_vectors(cols, J_ref)
    v, g = list(v), list(g)
    y, gr = jvp_of(v), vjp_of(g)
    B = PC.BOUND[ft]
    fy, fg, fa = PC.mixed_fractions(y, gr, cols, J_ref, kept, B)
    assert max(fy, fg, fa) < 1.0
    for j in range(6):
        bad = jvp_of([None if i == j else v[i] for i in range(6)])
        f = PC.mixed_fractions(bad, gr, cols, J_ref, kept, B)
        assert f[0] > 1.0 and f[2] > 1.0, ("dropped", scheme.WRT[j], f)
    for i, j in ((0, 1), (2, 3), (4, 5), (1, 2)):
        sw = list(v)
        sw[i], sw[j] = sw[j], sw[i]
        f = PC.mixed_fractions(jvp_of(sw), gr, cols, J_ref, kept, B)
        assert f[0] > 1.0 and f[2] > 1.0, ("swapped", scheme.WRT[i], scheme.WRT[j], f)
    for q in range(4):
        bad = vjp_of([-g[i] if i == q else g[i] for i in range(4)])
        f = PC.mixed_fractions(y, bad, cols, J_ref, kept, B)
        assert f[1] > 1.0 and f[2] > 1.0, ("negated", scheme.OUT[q], f)


# ---- the NaN rule ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_a_nan_poisons_every_output_of_its_point_only(host, oracle, ft, name):
    """A NaN in a state input, in a given tangent or in a given cotangent value of one point of 130: every product and every tendency of that point is NaN, every
    other point keeps its bits."""
    scheme = SCHEMES[name]
    case, which = scheme.INTERIOR
    cols, J_ref, _, _ = scheme.reference(case, which)
    cols = [np.array(c[:130]) for c in cols]
    _, hd = PC.head(scheme, ft, case)
    _, v, g, *_ = PC.mixed_vectors(cols, J_ref[:, :, :130])
    v, g = [np.array(a) for a in v], [np.array(a) for a in g]
    y0, ty0, _ = PC.host_jvp(host, scheme.entry, ft, hd, cols, v)
    g0, tg0, _ = PC.host_vjp(host, scheme.entry, ft, hd, cols, g)
    others = np.arange(130) != 77

    def poisoned(got, clean):
        return all(np.isnan(a[:, 77]).all() and _same_bits(a[:, others], b[:, others]) for a, b in zip(got, clean))
    for j in range(7):
        bad = [np.array(c) for c in cols]
        bad[j][77] = np.nan
        assert poisoned(PC.host_jvp(host, scheme.entry, ft, hd, bad, v)[:2], (y0, ty0)), ("state", j)
        assert poisoned(PC.host_vjp(host, scheme.entry, ft, hd, bad, g)[:2], (g0, tg0)), ("state", j)
    for j in range(6):
        bad = [np.array(a) for a in v]
        bad[j][77] = np.nan
        assert poisoned(PC.host_jvp(host, scheme.entry, ft, hd, cols, bad)[:2], (y0, ty0)), ("tangent", j)
    for q in range(4):
        bad = [np.array(a) for a in g]
        bad[q][77] = np.nan
        assert poisoned(PC.host_vjp(host, scheme.entry, ft, hd, cols, bad)[:2], (g0, tg0)), ("cotangent", q)
        for k in (1, 2):        # more than one pass: the tendencies are stored in the first, the gradients in every one
            assert poisoned(PC.host_vjp(host, scheme.entry, ft, hd, cols, bad, k=k)[:2], (g0, tg0)), ("cotangent", q, k)


# ---- statuses of the entry mirrors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", ["sb2006", "mp1m"])
def test_statuses_of_the_entry_mirrors(host, oracle, ft, name):
    scheme = SCHEMES[name]
    case, which = scheme.INTERIOR
    cols = [c[:8] for c in scheme.reference(case, which)[0]]
    mp, hd = PC.head(scheme, ft, case)
    one = np.ones(8)
    BAD = _abi.CMX_ERR_BAD_ARG
    # the table itself NULL; no output column at all
    assert PC.host_jvp(host, scheme.entry, ft, hd, cols, [one] * 6, table=False)[2] == BAD
    assert PC.host_vjp(host, scheme.entry, ft, hd, cols, [one] * 4, table=False)[2] == BAD
    assert PC.host_jvp(host, scheme.entry, ft, hd, cols, [one] * 6, want=[False] * 4, with_tendencies=False)[2] == BAD
    assert PC.host_vjp(host, scheme.entry, ft, hd, cols, [one] * 4, want=[False] * 6, with_tendencies=False)[2] == BAD
    # every member NULL is allowed: zeros
    y, _, rc = PC.host_jvp(host, scheme.entry, ft, hd, cols, [None] * 6)
    assert rc >= 0 and np.all(y == 0.0)
    gr, _, rc = PC.host_vjp(host, scheme.entry, ft, hd, cols, [None] * 4)
    assert rc >= 0 and np.all(gr == 0.0)
    # a flag the entry does not know
    bad_flags = C.c_uint32(1 << 17)
    for call, arg in ((PC.host_jvp, [one] * 6), (PC.host_vjp, [one] * 4)):
        assert call(host, scheme.entry, ft, (hd[0], hd[1], bad_flags), cols, arg)[2] == BAD


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("stem", ["cmx_sb2006_warm_rain", "cmx_mp1m"])
@pytest.mark.parametrize("product", ["jvp", "vjp", "jacobian"])
def test_argument_statuses_of_the_library_entries_without_gpu(ft, stem, product):
    """The twelve entries of libcmx.so: the statuses of the scheme's Jacobian entry in its order, the table itself NULL (the products; the Jacobian entry takes
    no table, its result table is jac[24]), no output column at all.  Every call below returns before any HIP runtime call."""
    from cmx import _lib
    from cmx import parameters as P
    fn = getattr(_lib.lib(), f"{stem}_{product}_{ft}")
    BAD, UNS, OK = _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED, _abi.CMX_OK
    sb = stem == "cmx_sb2006_warm_rain"
    mp, tps = (P.WarmRainParams2M(ft, True) if sb else P.Microphysics1MParams(ft)), P.ThermodynamicsParameters(ft)
    good = _abi.CMX_SB2006_LIMITED if sb else mp.flags
    n_in, n_out = {"jvp": (6, 4), "vjp": (4, 6), "jacobian": (0, 24)}[product]
    seven = [C.c_void_p(4096 + 64 * k) for k in range(7)]
    table = (C.c_void_p * n_in)(*[8192 + 64 * k for k in range(n_in)])
    res = (C.c_void_p * n_out)(*[16384 + 64 * k for k in range(n_out)])
    tend = (C.c_void_p * 4)(*[32768 + 64 * k for k in range(4)])
    nores, notend, notable = (C.c_void_p * n_out)(), (C.c_void_p * 4)(), (C.c_void_p * n_in)()
    huge = 16 * 0x7fffffff + 1

    def call(flags=good, n=8, cols=seven, p=table, r=res, t=tend, w=mp, th=tps):
        return fn(C.byref(w.c) if w is not None else None, C.byref(th) if th is not None else None, flags, n, *cols, *([p] if n_in else []), r, t, None)
    assert call(w=None) == BAD and call(th=None) == BAD                                   # no parameters
    assert call(n=-1) == BAD and call(n=huge) == UNS and call(n=0) == OK                   # the count rule
    assert call(n=0, cols=[None] * 7, p=None, r=None, t=None) == OK                        # n = 0 returns before the columns matter
    assert call(flags=1 << 17) == BAD and call(flags=1 << 31) == BAD                       # an unknown bit
    assert call(flags=1 << 17, n=0) == (OK if sb else BAD)                                 # SB2006: n = 0 first; 1-moment: the flags first, as its Jacobian entry
    for k in range(7):                                                                     # a NULL input column
        assert call(cols=seven[:k] + [None] + seven[k + 1:]) == BAD, k
    assert not n_in or call(p=None) == BAD                                                 # the tangent / cotangent table itself
    assert call(r=None, t=None) == BAD and call(r=nores, t=None) == BAD and call(r=nores, t=notend) == BAD and call(r=None, t=notend) == BAD    # no output
    del notable
