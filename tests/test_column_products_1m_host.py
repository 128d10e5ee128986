"""J v and Jᵀḡ of the 1-moment column step with sedimentation (include/cmx.h §(27)) in the HOST build tests/native/column_products_1m_host.cpp — the scheme
header the device kernels run (csrc/cmx_mp1m_column_jac.hpp) over columns on the CPU, so the mathematics is tested without a GPU: the four dual fall speeds
and fluxes, the coupling of a level with the one above, the two precipitation rows, the adjoint.  Columns, reference (central differences of the Float64
oracle's column step along v), measure and the 1 % condition: tests/column_products_1m_cases.py.  tests/test_column_products_1m_gpu.py repeats the
assertions through the C ABI on the device."""
import subprocess

import numpy as np
import pytest

import column_products_1m_cases as CC
from column_products_1m_cases import CASE_IDS, CASES, MAIN_CASE, WHICH, host  # noqa: F401
from jacobian_host_build import REPO, _build, _same_bits
import jacobian_products_cases as PC
from cmx import _abi

FTS = ["f64", "f32"]
SMALL = ["n1", "n2", "n3"]


def _products(host, ft, ref, **kw):
    case = ref["case"]
    jv, jp, tend, pr, rc = CC.host_jvp(host, ft, case, ref["inv_dz"], ref["cols"], ref["v"])
    grad, tend2, pr2, rc2 = CC.host_vjp(host, ft, case, ref["inv_dz"], ref["cols"], ref["g"], ref["pbar"], **kw)
    return jv, jp, grad, (tend, pr, tend2, pr2), (rc, rc2)


# ---- the reference alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_oracle_alone_stays_under_the_cap(oracle, case, which):
    """The set-aside criterion comes from the reference alone; at most 1 % of the points and of the columns of the large set may be set aside, none of a
    small set, and no precipitation row."""
    ref = CC.reference_unchecked(case, which, "n7")
    pts, cls = CC.set_aside_shares(ref)
    print(f"{case} {which} n7: set aside {int((~ref['kept']).sum())} of {ref['kept'].size} points ({pts:.4f}), {int((~ref['keptc']).sum())} of "
          f"{ref['keptc'].size} columns ({cls:.4f}), worst t-vs-4t disagreement {ref['worst']:.3g}, on kept points {ref['worst_kept']:.3g}; "
          f"columns with rain / snow at the surface {(ref['sp'] > 0).mean(axis=1)}")
    assert pts <= CC.MAX_SET_ASIDE and cls <= CC.MAX_SET_ASIDE
    assert ref["keptp"].all()
    assert (ref["s"] > 0).all() and (ref["sp"] >= 0).all() and ((ref["sp"] > 0).mean(axis=1) > 0.8).all()      # every row is resolved; most columns carry rain, resp. snow, at the surface
    if case == MAIN_CASE:
        for shape in SMALL:
            assert CC.set_aside_shares(CC.reference_unchecked(case, which, shape)) == (0.0, 0.0), shape


# ---- J v against the differenced oracle, the adjoint identity per column ---------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_products_match_the_differenced_oracle_and_are_adjoint(host, oracle, ft, case, which):
    """Every parameter case (the compile-time and the run-time-flags instantiation, the general Γ: the return value names what ran) on the cold and the warm set."""
    ref = CC.reference(case, which, "n7")
    jv, jp, grad, _, rc = _products(host, ft, ref)
    assert rc == (CC.KIND[case],) * 2
    CC.assert_products(ft, ref, jv, jp, grad, "host")


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("shape", SMALL)
def test_small_columns(host, oracle, ft, shape, which):
    """One level (every cell is top and surface), two, and two columns of three."""
    ref = CC.reference(MAIN_CASE, which, shape)
    jv, jp, grad, _, _ = _products(host, ft, ref)
    CC.assert_products(ft, ref, jv, jp, grad, "host")


@pytest.mark.parametrize("which", WHICH)
def test_the_measure_rejects_wrong_products(host, oracle, which):
    """A tangent column scaled by 1.1, the flux terms dropped (the pointwise J v in the place of the column's) and the level-above term shifted by one level
    are each rejected; so are a precipitation row with the wrong sign and an adjoint identity without the precipitation terms."""
    ref = CC.reference(MAIN_CASE, which, "n7")
    jv, jp, grad, _, _ = _products(host, "f64", ref)
    B = CC.BOUND["f64"]
    n_col, n_lev = ref["n_col"], ref["n_lev"]
    # a tangent column scaled by 1.1: every one of the six
    for j in range(6):
        v = [np.asarray(a) * (1.1 if i == j else 1.0) for i, a in enumerate(ref["v"])]
        wrong = CC.host_jvp(host, "f64", MAIN_CASE, ref["inv_dz"], ref["cols"], v)
        assert max(CC.jvp_fractions(ref, wrong[0], wrong[1], B)) > 1.0, j
    # the flux terms dropped: the pointwise J v (inv_dz = 0)
    pointwise = CC.host_jvp(host, "f64", MAIN_CASE, 0 * ref["inv_dz"], ref["cols"], ref["v"])[0]
    assert CC.jvp_fractions(ref, pointwise, jp, B)[0] > 1.0
    # the level-above term shifted by one level: y − pointwise is the flux part; its inflow share taken from the wrong level
    flux = (jv - pointwise).reshape(4, n_col, n_lev)
    shifted = pointwise + np.roll(flux, 1, axis=2).reshape(4, -1)
    assert CC.jvp_fractions(ref, shifted, jp, B)[0] > 1.0
    assert CC.jvp_fractions(ref, jv, -jp, B)[1] > 1.0
    assert CC.jvp_fractions(ref, jv, jp[::-1], B)[1] > 1.0          # rain and snow rows exchanged
    assert CC.adjoint_fraction(ref, jv, jp, np.roll(grad, 1, axis=1), B) > 1.0
    assert CC.adjoint_fraction(ref, jv, 0 * jp, grad, B) > 1.0      # without the precipitation terms the identity does not hold


# ---- structure, exact ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_a_seed_at_one_level_reaches_its_own_level_and_one_neighbour_only(host, oracle, ft):
    """A tangent confined to level k changes J v at levels k and k − 1 of that column only; a cotangent at level k reaches gradients at levels k and k + 1
    only; nothing crosses from the top level of column c to level 0 of column c + 1, neighbours in the flat index."""
    ref = CC.reference(MAIN_CASE, "cold", "n3")
    n_col, n_lev = ref["n_col"], ref["n_lev"]
    zero = np.zeros((n_col, n_lev))
    for c in range(n_col):
        for k in range(n_lev):
            at = zero.copy()
            at[c, k] = 1.0
            jv, jp, _, _, _ = CC.host_jvp(host, ft, MAIN_CASE, ref["inv_dz"], ref["cols"], [np.asarray(v).reshape(n_col, n_lev) * at for v in ref["v"]])
            touched = (jv != 0).any(axis=0).reshape(n_col, n_lev)
            allowed = zero.astype(bool)
            allowed[c, max(k - 1, 0):k + 1] = True
            assert not (touched & ~allowed).any() and touched[c, k] and (k == 0 or touched[c, k - 1]), (c, k, touched)
            assert ((jp != 0) == ((np.arange(n_col) == c) & (k == 0))[None]).all(), (c, k, jp)
            grad, _, _, _ = CC.host_vjp(host, ft, MAIN_CASE, ref["inv_dz"], ref["cols"], [np.asarray(g).reshape(n_col, n_lev) * at for g in ref["g"]], None)
            touched = (grad != 0).any(axis=0).reshape(n_col, n_lev)
            allowed = zero.astype(bool)
            allowed[c, k:k + 2] = True
            assert not (touched & ~allowed).any() and touched[c, k] and (k == n_lev - 1 or touched[c, k + 1]), (c, k, touched)
    # a precipitation cotangent reaches level 0 of its column only, in the input its flux depends on
    for c in range(n_col):
        for r, j in ((0, CC.WRT.index("q_rai")), (1, CC.WRT.index("q_sno"))):
            pbar = [None, None]
            pbar[r] = np.where(np.arange(n_col) == c, 1.0, 0.0)
            grad, _, _, _ = CC.host_vjp(host, ft, MAIN_CASE, ref["inv_dz"], ref["cols"], [None] * 4, pbar)
            touched = (grad != 0).reshape(6, n_col, n_lev)
            assert touched[j, c, 0] and touched.sum() == 1, (c, r, touched)


@pytest.mark.parametrize("ft", FTS)
def test_j_and_its_transpose_from_unit_seeds_agree_entry_by_entry(host, oracle, ft):
    """A column of three levels: J (14 rows: 4 outputs per level and the two precipitation fluxes; 18 columns) column by column from unit tangents and row by
    row from unit cotangents, within the entry bound B·s'_i of the input-scaled measure."""
    ref = CC.reference(MAIN_CASE, "warm", "n3")
    n_lev = ref["n_lev"]
    cols = [np.asarray(c)[:1] for c in ref["cols"]]
    unit = lambda k: np.where(np.arange(n_lev) == k, 1.0, 0.0)[None]  # noqa: E731
    Jc, Jr = np.zeros((4 * n_lev + 2, 6 * n_lev)), np.zeros((4 * n_lev + 2, 6 * n_lev))
    for k in range(n_lev):
        for j in range(6):
            jv, jp, _, _, _ = CC.host_jvp(host, ft, MAIN_CASE, ref["inv_dz"], cols, [unit(k) if i == j else None for i in range(6)])
            Jc[:-2, 6 * k + j] = jv.T.reshape(-1)          # row 4·level + output
            Jc[-2:, 6 * k + j] = jp[:, 0]
        for q in range(4):
            grad, _, _, _ = CC.host_vjp(host, ft, MAIN_CASE, ref["inv_dz"], cols, [unit(k) if i == q else None for i in range(4)], None)
            Jr[4 * k + q] = grad.T.reshape(-1)             # column 6·level + input
    for r in range(2):
        Jr[-2 + r] = CC.host_vjp(host, ft, MAIN_CASE, ref["inv_dz"], cols, [None] * 4, [np.ones(1) if i == r else None for i in range(2)])[0].T.reshape(-1)
    x = np.stack([np.asarray(c)[0] for c in ref["cols"][1:]]).T.reshape(-1)
    s = np.concatenate([ref["s"][:, :n_lev].T.reshape(-1), ref["sp"][:, 0]])
    frac = np.abs(Jc - Jr) * np.abs(x)[None] / (CC.BOUND[ft] * s[:, None])
    print(f"{ft}: J from unit tangents against J from unit cotangents, worst used fraction of the entry bound {frac.max():.3g}; {int((Jc != 0).sum())} non-zero entries")
    assert frac.max() < 1.0
    # upper bidiagonal in the level index
    for k in range(n_lev):
        for m in range(n_lev):
            if m not in (k, k + 1):
                assert not Jc[4 * k:4 * k + 4, 6 * m:6 * m + 6].any() and not Jr[4 * k:4 * k + 4, 6 * m:6 * m + 6].any()
    assert not Jc[-2:, 6:].any() and not Jr[-2:, 6:].any() and Jc[-2, :6].any() and Jc[-1, :6].any()


# ---- bit identities --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_value_parts_are_the_plain_instantiation(host, oracle, ft, case):
    """Requested tendencies and precipitation fluxes of both entries equal the plain instantiation's (the operations of the primal kernel), bit for bit —
    and that one follows the Float64 oracle."""
    ref = CC.reference(case, "cold", "n7")
    want, wantp, rc = CC.host_plain(host, ft, case, ref["inv_dz"], ref["cols"])
    assert rc == CC.KIND[case]
    _, _, _, (tend, pr, tend2, pr2), _ = _products(host, ft, ref)
    assert _same_bits(tend, want) and _same_bits(tend2, want) and _same_bits(pr, wantp) and _same_bits(pr2, wantp)
    import oracle_binding
    y, p = CC.oracle_column(oracle_binding, case, ref["inv_dz"], ref["cols"])
    tol = 1e-9 if ft == "f64" else 2e-3
    scale = np.abs(y).max(axis=1, keepdims=True)
    assert (np.abs(want - y) <= tol * scale).all() and (np.abs(wantp - p) <= tol * np.abs(p).max(axis=1, keepdims=True)).all()


@pytest.mark.parametrize("ft", FTS)
def test_a_gradient_does_not_depend_on_what_else_is_requested_or_on_k(host, oracle, ft):
    ref = CC.reference(MAIN_CASE, "cold", "n7")
    args = (host, ft, MAIN_CASE, ref["inv_dz"], ref["cols"])
    full, _, _, rc = CC.host_vjp(*args, ref["g"], ref["pbar"])
    for k in (1, 2, 3, 6):
        assert _same_bits(CC.host_vjp(*args, ref["g"], ref["pbar"], k=k)[0], full), k
    rng = np.random.default_rng(3)
    for trial in range(6):
        want = rng.random(6) < 0.5
        want[trial] = True
        got = CC.host_vjp(*args, ref["g"], ref["pbar"], want=tuple(want), with_primal=bool(trial % 2))[0]
        for j in range(6):
            assert _same_bits(got[j], full[j]) if want[j] else (got[j] == -7.0).all(), (trial, j)
    jv, jp, _, _, _ = CC.host_jvp(*args, ref["v"])
    got = CC.host_jvp(*args, ref["v"], want=(False, True, False, True), want_precip=(False, True), with_primal=False)
    assert _same_bits(got[0][1], jv[1]) and _same_bits(got[0][3], jv[3]) and (got[0][0] == -7.0).all() and (got[1][0] == -7.0).all() and (got[2] == -7.0).all()
    assert _same_bits(got[1][1], jp[1])


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_without_sedimentation_the_products_are_the_pointwise_ones(host, oracle, ft, case):
    """inv_dz = 0: the flux terms multiply by an exact zero, and J v and Jᵀḡ equal the pointwise entries' (tests/native/derivatives_host.cpp) under == on
    states with finite flux tangents."""
    ref = CC.reference(case, "warm", "n7")
    zero = np.zeros_like(ref["inv_dz"])
    jv, jp, _, _, _ = CC.host_jvp(host, ft, case, zero, ref["cols"], ref["v"])
    grad, _, _, _ = CC.host_vjp(host, ft, case, zero, ref["cols"], ref["g"], None)
    flat = [np.asarray(c).reshape(-1) for c in ref["cols"]]
    point = _build("derivatives_host")
    mp, head = PC.head(PC.MP1M, ft, case[0])
    pjv = PC.host_jvp(point, "mp1m", ft, head, flat, [np.asarray(v).reshape(-1) for v in ref["v"]])[0]
    pgrad = PC.host_vjp(point, "mp1m", ft, head, flat, [np.asarray(g) for g in ref["g"]])[0]
    assert np.isfinite(jv).all() and np.isfinite(jp).all()
    assert (jv == pjv).all() and (grad == pgrad).all()


# ---- the NaN rule and the argument checks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_the_nan_rule(host, oracle, ft):
    """A NaN in a state input, a tangent or a cotangent of a point → every output of that point; a NaN in ρ or a species' q reaches the cell below through
    that species' flux exactly as in the primal; a NaN in ḡ or ρ of the level below reaches x̄ through λ (ρ: as a non-finite value).  No other point changes, bit for bit."""
    ref = CC.reference(MAIN_CASE, "cold", "n2")      # 32 columns of 2 levels
    n_col, n_lev = ref["n_col"], ref["n_lev"]
    args = (host, ft, MAIN_CASE, ref["inv_dz"], ref["cols"])
    cjv, cjp, ctend, cpr, _ = CC.host_jvp(*args, ref["v"])
    cgrad, _, _, _ = CC.host_vjp(*args, ref["g"], ref["pbar"])

    def with_nan(arrays, j, at):
        out = [np.array(a, dtype=np.float64).reshape(n_col, n_lev) for a in arrays]
        out[j][at] = np.nan
        return out
    top, bottom = (5, 1), (5, 0)
    i_top, i_bot = 5 * n_lev + 1, 5 * n_lev
    others = lambda *hit: ~np.isin(np.arange(n_col * n_lev), hit)  # noqa: E731
    for j in range(7):
        bad = with_nan(ref["cols"], j, top)
        jv, jp, tend, pr, _ = CC.host_jvp(host, ft, MAIN_CASE, ref["inv_dz"], bad, ref["v"])
        grad, tend2, _, _ = CC.host_vjp(host, ft, MAIN_CASE, ref["inv_dz"], bad, ref["g"], ref["pbar"])
        want, wantp, _ = CC.host_plain(host, ft, MAIN_CASE, ref["inv_dz"], bad)
        assert np.isnan(jv[:, i_top]).all() and np.isnan(grad[:, i_top]).all() and np.isnan(tend[:, i_top]).all(), j
        assert _same_bits(tend, want) and _same_bits(tend2, want) and _same_bits(pr, wantp), j
        assert (np.isnan(jv) == np.isnan(want)).all(), j           # the flux NaN reaches the cell below in J v exactly where it does in the primal
        # ρ poisons all four fluxes, q_s its own
        hit_below = np.isnan(want[:, i_bot])
        assert (hit_below == np.array([j == 0 or j == 3 + s for s in range(4)])).all(), (j, hit_below)
        assert _same_bits(jv[:, others(i_top, i_bot)], cjv[:, others(i_top, i_bot)]) and _same_bits(jp, cjp), j
        # a NaN at level 0 reaches the precipitation outputs of its column: ρ both, q_rai and q_sno their own
        bad = with_nan(ref["cols"], j, bottom)
        jv, jp, _, pr, _ = CC.host_jvp(host, ft, MAIN_CASE, ref["inv_dz"], bad, ref["v"])
        assert (np.isnan(jp[:, 5]) == np.array([j in (0, 5), j in (0, 6)])).all() and (np.isnan(pr[:, 5]) == np.isnan(jp[:, 5])).all(), j
        assert np.isnan(jv[:, i_bot]).all() and _same_bits(jv[:, others(i_bot)], cjv[:, others(i_bot)]), j
        # Jᵀḡ: the point above receives nothing from the NaN point but ρ of the level below, which enters λ of the point above
        grad = CC.host_vjp(host, ft, MAIN_CASE, ref["inv_dz"], bad, ref["g"], ref["pbar"])[0]
        assert np.isnan(grad[:, i_bot]).all() and _same_bits(grad[:, others(i_top, i_bot)], cgrad[:, others(i_top, i_bot)]), j
        # (g_{k−1} is the primal's: max(0, NaN) = 0 and its reciprocal +Inf, so λ and the flux terms above are non-finite, not necessarily NaN)
        assert (~np.isfinite(grad[2:, i_top])).all() == (j == 0) and (~np.isfinite(grad[2:, i_top])).any() == (j == 0), j
        assert _same_bits(grad[:2, i_top], cgrad[:2, i_top]), j
    for j in range(6):
        jv, jp, tend, _, _ = CC.host_jvp(*args, with_nan(ref["v"], j, top))
        assert np.isnan(jv[:, i_top]).all() and np.isnan(tend[:, i_top]).all() and _same_bits(jv[:, others(i_top, i_bot)], cjv[:, others(i_top, i_bot)]), j
        # the NaN tangent reaches Ḟ of its own species by plain IEEE arithmetic, and the cell below through it
        assert (np.isnan(jv[:, i_bot]) == np.array([j == 2 + s for s in range(4)])).all(), j
    for q in range(4):
        grad, tend, _, _ = CC.host_vjp(*args, with_nan(ref["g"], q, bottom), ref["pbar"])
        assert np.isnan(grad[:, i_bot]).all() and np.isnan(tend[:, i_bot]).all() and _same_bits(grad[:, others(i_top, i_bot)], cgrad[:, others(i_top, i_bot)]), q
        # ḡ_q of the level below → λ[q] → the gradient of q_s, s = q, alone
        assert (np.isnan(grad[:, i_top]) == np.array([j == 2 + q for j in range(6)])).all(), q
    for r in range(2):
        pbar = [np.array(p) for p in ref["pbar"]]
        pbar[r][5] = np.nan
        grad = CC.host_vjp(*args, ref["g"], pbar)[0]
        assert np.isnan(grad[:, i_bot]).all() and _same_bits(grad[:, others(i_bot)], cgrad[:, others(i_bot)]), r
    if ft == "f64":      # Float64: ρ ≤ 0 is poisoned like a NaN ρ
        bad = [np.array(a, dtype=np.float64) for a in ref["cols"]]
        bad[0][top] = 0.0
        jv, jp, tend, pr, _ = CC.host_jvp(host, ft, MAIN_CASE, ref["inv_dz"], bad, ref["v"])
        assert np.isnan(jv[:, i_top]).all() and np.isnan(tend[:, i_top]).all() and np.isnan(jv[:, i_bot]).all()


def test_argument_checks(host, oracle):
    ref = CC.reference(MAIN_CASE, "cold", "n3")
    args = ("f64", MAIN_CASE, ref["inv_dz"], ref["cols"])
    BAD, UNS = _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED
    flags = CC.params("f64", MAIN_CASE)[0].flags
    for f, want in ((flags | _abi.CMX_1M_SED_SNOW_OBLATE | _abi.CMX_1M_SED_SNOW_PROLATE, BAD), (flags | _abi.CMX_1M_SED_SNOW_OBLATE, UNS),
                    (flags | _abi.CMX_1M_SED_SNOW_PROLATE, UNS), (flags | (1 << 30), BAD)):
        assert CC.host_jvp(host, *args, ref["v"], override_flags=f)[-1] == want, f
        assert CC.host_vjp(host, *args, ref["g"], ref["pbar"], override_flags=f)[-1] == want, f
    # no output at all
    assert CC.host_jvp(host, *args, ref["v"], want=(False,) * 4, want_precip=(False, False), with_primal=False)[-1] == BAD
    assert CC.host_vjp(host, *args, ref["g"], ref["pbar"], want=(False,) * 6, with_primal=False)[-1] == BAD
    # a NULL tangent table is a zero tangent, a NULL cotangent table no cotangent: exact zeros
    jv, jp, tend, _, rc = CC.host_jvp(host, *args, None)
    assert rc >= 0 and not jv.any() and not jp.any() and np.isfinite(tend).all()
    grad, _, _, rc = CC.host_vjp(host, *args, None, None)
    assert rc >= 0 and not grad.any() and not np.signbit(grad).any()


# ---- the stand-alone program -----------------------------------------------------------------------------------------------------------------------
def test_the_stand_alone_program_runs(tmp_path):
    """tests/native/column_products_1m_host.cpp with its own main (the program to build with host sanitizer flags): compiled plainly here, run on the default
    parameter structs written as raw bytes; it checks the adjoint identity over whole columns itself."""
    exe = tmp_path / "column_products_1m"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DCMX_COLUMN_PRODUCTS_1M_MAIN", "-o", str(exe),
                    str(REPO / "tests" / "native" / "column_products_1m_host.cpp")], check=True)
    files = []
    for ft in ("f32", "f64"):
        mp, tps, stokes, cr, ci = CC.params(ft, MAIN_CASE)
        path = tmp_path / f"params_{ft}.bin"
        path.write_bytes(b"".join(bytes(memoryview(s)) for s in (mp.c, tps, stokes, cr, ci)) + int(mp.flags).to_bytes(4, "little"))
        files.append(str(path))
    r = subprocess.run([str(exe), *files], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
