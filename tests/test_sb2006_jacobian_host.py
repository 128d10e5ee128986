"""The SB2006 warm-rain Jacobian without a GPU (include/cmx.h §(14), cmx.warm_rain_jacobian_2m):

  * the dual instantiation of the device point function (csrc/cmx_dual.hpp, csrc/cmx_sb2006_jacobian.hpp) compiled by g++ for the host
    (tests/native/derivatives_host.cpp) against central differences of the Float64 oracle — tests/jacobian_cases.py has the states, the reference and the
    measure — at the reference's own bound 1e-5 (test/ad_compat_tests.jl:163) in Float64 and the project's Float32 bound 1e-3 in every row in Float32 —
    except dn_rai_dt with the perturbed parameter set, which misses it at ONE state (2.2e-3 here, 2.3e-3 on the device) and is held entry by entry to the
    bound its evaporation share earns from the oracle's own Float32-against-Float64 spread of the evaporation rate (jacobian_cases.float32_bound);
  * the same parity in the second, input-scaled measure of tests/jacobian_cases.py (every entry weighted by |x_j|: the T and number columns, which the
    per-row scale hides behind the q columns) at the same two bounds, no exception: host build worst 2.3e-8 in Float64, 5.2e-6 in Float32;
  * that both measures can fail: every input column scaled by 1.1, zeroed or negated is rejected, every structurally non-zero entry reaches 1 % of its
    row in one of the measures on the interior set, and every such entry wrong by 0.2 % / 20 % is rejected;
  * the value parts against the plain instantiation, bit for bit; the columns against the tangent width K, bit for bit;
  * finiteness at the reference's boundary state and on every present / absent combination of the four species;
  * the argument statuses of the two entries and the Python wrapper's errors.

The host build proves the derivative RULES (its transcendentals are libm's, not the hardware's); tests/test_sb2006_jacobian_gpu.py repeats the parity
assertions on the device."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import jacobian_cases as JC
import jacobian_host_build as JH
from jacobian_host_build import NPT, _same_bits, host_fixture
import cmx
from cmx import _abi, _lib, synthetic
from cmx import parameters as P

host = host_fixture()


def _head(ft, wr, limited):
    return C.byref(wr.c), C.byref(P.ThermodynamicsParameters(ft)), C.c_uint32(_abi.CMX_SB2006_LIMITED if limited else 0)


def host_jacobian(host, ft, wr, limited, cols, wrt=JC.WRT, k=0, with_tendencies=True):
    """([4, len(wrt), n] Jacobian, [4, n] tendencies, status) of the host build; wrt: names in any order."""
    return JH.host_jacobian(host, "sb2006", ft, _head(ft, wr, limited), cols, JC.WRT, wrt, k=k, with_tendencies=with_tendencies)


def host_plain(host, ft, wr, limited, cols):
    return JH.host_plain(host, "sb2006", ft, _head(ft, wr, limited), cols)


# ---- parity against the finite-difference reference ---------------------------------------------------------------------------------------------
CASES = [(True, False), (False, False), (True, True)]        # (limited, perturbed exponents → the general-exponent instantiation)


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("limited,perturbed", CASES)
def test_host_jacobian_matches_central_differences_of_the_oracle(host, oracle, ft, limited, perturbed):
    """Float64: every row of every kept state within the reference's own 1e-5.  Float32, same Float64 reference: every row within 1e-3, except dn_rai_dt
    with the perturbed parameter set, held entry by entry to jacobian_cases.float32_bound (worst values observed: DESIGN.md §6).  Input-scaled measure:
    every (row, column) within the same 1e-5 / 1e-3, no exception."""
    wr = JC.warm_rain_params(ft, limited, JC.perturbed_overrides() if perturbed else None)
    for which in ("interior", "points"):
        J, _, rc = host_jacobian(host, ft, wr, limited, JC.reference(limited, perturbed, which)[0])
        assert rc == (0 if perturbed else 1)                 # which instantiation ran: the one sb_integer_exponents selects
        JC.assert_parity(ft, J, limited, perturbed, which, "host")


# ---- the two measures can fail ------------------------------------------------------------------------------------------------------------------
MUTATIONS = (("scaled by 1.1", 1.1), ("zeroed", 0.0), ("negated", -1.0))
# the entries that do not exist: dq_lcl_dt does not see n_rai, dn_lcl_dt sees neither T, q_tot nor n_rai (no condensation term in the number)
STRUCTURAL_ZEROS = {("dq_lcl_dt", "n_rai"), ("dn_lcl_dt", "T"), ("dn_lcl_dt", "q_tot"), ("dn_lcl_dt", "n_rai")}


def _rejected(ft, M, limited, perturbed, which):
    try:
        JC.assert_parity(ft, M, limited, perturbed, which, "mutated", report=False)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("limited,perturbed", CASES)
def test_a_corrupted_column_is_rejected(host, oracle, ft, limited, perturbed):
    """Each of the six input columns of the host-build Jacobian, whole, scaled by 1.1, zeroed or negated: assert_parity raises, in both float types, on
    the interior set and on the pinned states.  (The row measure alone accepts the n_lcl and n_rai columns scaled, zeroed or negated in both float types
    and the T column scaled in Float32: test_the_row_measure_alone_does_not_see_the_number_columns.)"""
    wr = JC.warm_rain_params(ft, limited, JC.perturbed_overrides() if perturbed else None)
    for which in ("interior", "points"):
        cols, J_ref, kept, _ = JC.reference(limited, perturbed, which)
        J, _, _ = host_jacobian(host, ft, wr, limited, cols)
        assert not _rejected(ft, J, limited, perturbed, which)
        for j, name in enumerate(JC.WRT):
            assert np.any(J_ref[:, j, kept] != 0), name
            for kind, f in MUTATIONS:
                M = np.array(J)
                M[:, j] *= NPT[ft](f)
                assert _rejected(ft, M, limited, perturbed, which), (which, name, kind)


@pytest.mark.parametrize("limited,perturbed", CASES)
def test_the_row_measure_alone_does_not_see_the_number_columns(host, oracle, limited, perturbed):
    """Why the second measure exists: with the n_lcl column 10 % wrong at every state the per-row measure stays inside the FLOAT64 bound, with the n_rai
    column inside the Float32 one (2.5e-6 with the default parameters, 1.5e-5 with the perturbed set); the input-scaled one shows 0.1/1.1."""
    cols, J_ref, kept, _ = JC.reference(limited, perturbed, "interior")
    J, _, _ = host_jacobian(host, "f64", JC.warm_rain_params("f64", limited, JC.perturbed_overrides() if perturbed else None), limited, cols)
    for name, ft in (("n_lcl", "f64"), ("n_rai", "f32")):
        M = np.array(J)
        M[:, JC.WRT.index(name)] *= 1.1
        assert max(JC.worst_rows(M, J_ref, kept, JC.OUT).values()) < JC.BOUND[ft], name
        assert abs(JC.worst_cells(M, J_ref, cols[1:], kept).max() - 0.1 / 1.1) < 1e-6, name


@pytest.mark.parametrize("limited,perturbed", CASES)
def test_every_entry_of_the_reference_is_resolved_by_the_interior_set(host, oracle, limited, perturbed):
    """From the reference alone: every structurally non-zero entry reaches at least 1 % of its row in one of the two measures at some kept state
    (jacobian_cases.assert_resolution prints the relative error each entry is resolved to), and the entries that are zero are the four that do not
    exist.  Then the same with the code under test: every such entry of the host-build Jacobian wrong by 0.2 % (Float64) or 20 % (Float32) at every state
    is rejected — twice the error the 1 % share promises to see."""
    cols, J_ref, kept, _ = JC.reference(limited, perturbed, "interior")
    share, nonzero = JC.assert_resolution(J_ref, cols[1:], kept, JC.OUT, JC.WRT, f"SB2006 limited={limited} perturbed={perturbed} interior")
    assert {(JC.OUT[i], JC.WRT[j]) for i, j in zip(*np.nonzero(~nonzero))} == STRUCTURAL_ZEROS
    for ft, f in (("f64", 1.002), ("f32", 1.2)):
        J, _, _ = host_jacobian(host, ft, JC.warm_rain_params(ft, limited, JC.perturbed_overrides() if perturbed else None), limited, cols)
        for i, j in zip(*np.nonzero(nonzero)):
            M = np.array(J)
            M[i, j] *= NPT[ft](f)
            assert _rejected(ft, M, limited, perturbed, "interior"), (ft, JC.OUT[i], JC.WRT[j], float(share[i, j]))


def test_input_scaled_error_edges():
    """A row with s'_i = 0 must be exactly zero; a non-finite entry gives Inf; the weights are the reference's state columns."""
    x = [np.array([2.0, 0.0, 1.0])] + [np.array([1e-4, 1e-4, 1e-4])] * 5
    J_ref = np.zeros((4, 6, 3))
    J_ref[0, 0], J_ref[0, 1] = 1.0, 3e4
    J = J_ref.copy()
    assert np.all(JC.input_scaled_error(J, J_ref, x) == 0)
    J[0, 0, 0] = 1.5                                     # s' = max(1.5·2, 3) = 3: error 0.5·2/3
    J[0, 0, 1] = 1.5                                     # x_0 = 0 at state 1: invisible in this measure (the row measure sees it)
    J[1, 0, 1] = 1e-30                                   # s' = 0 (x_0 = 0 and the reference row is zero): the row must be exactly zero
    J[2, 3, 0] = np.nan
    e = JC.input_scaled_error(J, J_ref, x)
    assert e[0, 0, 0] == pytest.approx(1.0 / 3.0) and e[0, 0, 1] == 0 and e[0, 1, 0] == 0
    assert e[1, 0, 1] == np.inf and np.all(e[1, 1:, 1] == 0) and np.all(e[1, :, [0, 2]] == 0)
    assert e[2, 3, 0] == np.inf and np.all(e[3] == 0)


# ---- the primal ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("limited", [True, False])
def test_value_parts_are_the_plain_instantiation_bit_for_bit(host, oracle, ft, limited):
    wr = JC.warm_rain_params(ft, limited)
    dt = {"f32": torch.float32, "f64": torch.float64}[ft]
    for cols in (JC.reference(limited)[0], [c.numpy() for c in synthetic.sb2006_state(4096, dtype=dt, seed=321)]):
        plain, rc = host_plain(host, ft, wr, limited, cols)
        assert rc == 1
        for wrt in (JC.WRT, ("q_rai",), ()):
            _, tend, _ = host_jacobian(host, ft, wr, limited, cols, wrt=wrt)
            assert _same_bits(tend, plain), wrt


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_columns_do_not_depend_on_the_tangent_width_or_the_selection(host, oracle, ft):
    """Each tangent is computed by the same operations whatever K is and whichever other inputs are seeded: K = 1, 2, 3, 4, 6, subsets in any order."""
    wr = JC.warm_rain_params(ft, True)
    cols = [c[:512] for c in JC.reference(True)[0]]
    full, _, _ = host_jacobian(host, ft, wr, True, cols)
    for k in (1, 2, 3, 4, 6):
        J, _, rc = host_jacobian(host, ft, wr, True, cols, k=k)
        assert rc == 1 and _same_bits(J, full), k
    for wrt in (("n_rai", "T"), ("q_lcl",), ("q_rai", "q_tot", "n_lcl", "T", "q_lcl")):
        J, _, _ = host_jacobian(host, ft, wr, True, cols, wrt=wrt)
        for kk, name in enumerate(wrt):
            assert _same_bits(J[:, kk], full[:, JC.WRT.index(name)]), (wrt, name)


# ---- finiteness ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("limited", [True, False])
def test_jacobian_is_finite_at_the_zero_rain_boundary(host, ft, limited):
    """ad_compat_tests.jl:167-174: Φ_au(τ) ∝ τ^0.7 has a vertical tangent at exactly zero rain with cloud present; the ϵ-gate keeps the Jacobian finite."""
    J, tend, _ = host_jacobian(host, ft, JC.warm_rain_params(ft, limited), limited, JC.points(JC.BOUNDARY))
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(tend))


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("limited", [True, False])
def test_jacobian_is_finite_with_absent_species(host, oracle, ft, limited):
    """The 16 present / absent combinations of (q_lcl, n_lcl, q_rai, n_rai) ∈ {0, interior value} at ρ = 1, T = 285, sub- and super-saturated: every entry
    is finite, and the column of an absent species is exactly zero — the input clamp max(0, x) passes no tangent at x = 0 and every gate behind it is a
    select."""
    qs = float(JC.q_sat(oracle, np.array([285.0]), np.array([1.0]))[0])
    states = []
    for sat in (0.7, 1.03):
        for present in itertools.product((0, 1), repeat=4):
            ql, nl, qr, nr = (v * p for v, p in zip((1e-3, 1e8, 5e-4, 1e4), present))
            states.append((1.0, 285.0, ql + qr + sat * qs, ql, nl, qr, nr))
    cols = JC.points(*states)
    J, tend, _ = host_jacobian(host, ft, JC.warm_rain_params(ft, limited), limited, cols)
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(tend))
    for name in ("q_lcl", "n_lcl", "q_rai", "n_rai"):
        j = JC.WRT.index(name)
        absent = cols[j + 1] == 0
        assert absent.sum() == 16 and np.all(J[:, j, absent] == 0), name


def test_a_nan_input_poisons_every_output_of_its_point(host, oracle):
    for ft in ("f64", "f32"):
        cols = [np.array(c[:16], dtype=NPT[ft]) for c in JC.reference(True)[0]]
        clean, ctend, _ = host_jacobian(host, ft, JC.warm_rain_params(ft, True), True, cols)
        for j in range(7):
            bad = [c.copy() for c in cols]
            bad[j][5] = np.nan
            J, tend, _ = host_jacobian(host, ft, JC.warm_rain_params(ft, True), True, bad)
            assert np.all(np.isnan(J[:, :, 5])) and np.all(np.isnan(tend[:, 5]))
            keep = np.arange(16) != 5
            assert _same_bits(J[:, :, keep], clean[:, :, keep]) and _same_bits(tend[:, keep], ctend[:, keep])


# ---- statuses and the wrapper's errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_argument_statuses_without_gpu(ft):
    """Every call below returns before any HIP runtime call."""
    lib = _lib.lib()
    fn = getattr(lib, f"cmx_sb2006_warm_rain_jacobian_{ft}")
    BAD, UNS, OK = _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED, _abi.CMX_OK
    wr, tps = P.WarmRainParams2M(ft, True), P.ThermodynamicsParameters(ft)
    seven = [C.c_void_p(4096 + 64 * k) for k in range(7)]
    jac = (C.c_void_p * _abi.CMX_SB2006_JAC_NCOL)(*[8192 + 64 * k for k in range(_abi.CMX_SB2006_JAC_NCOL)])
    tend = (C.c_void_p * 4)(*[16384 + 64 * k for k in range(4)])
    nojac, notend = (C.c_void_p * _abi.CMX_SB2006_JAC_NCOL)(), (C.c_void_p * 4)()
    huge = 16 * 0x7fffffff + 1

    def call(flags=_abi.CMX_SB2006_LIMITED, n=8, cols=seven, j=jac, t=tend, w=wr, th=tps):
        return fn(C.byref(w.c) if w is not None else None, C.byref(th) if th is not None else None, flags, n, *cols, j, t, None)
    assert call(w=None) == BAD and call(th=None) == BAD                                   # no parameters
    assert call(n=-1) == BAD and call(n=huge) == UNS and call(n=0) == OK                   # the count rule
    assert call(n=0, cols=[None] * 7, j=None, t=None) == OK                                # n = 0 returns before the columns matter …
    assert call(n=0, flags=1 << 7) == OK                                                   # … and before the flags, like the tendencies entry
    for k in range(7):                                                                     # a NULL input column
        assert call(cols=seven[:k] + [None] + seven[k + 1:]) == BAD, k
    assert call(j=None, t=None) == BAD and call(j=nojac, t=None) == BAD and call(j=nojac, t=notend) == BAD and call(j=None, t=notend) == BAD    # no output
    for bit in (_abi.CMX_VEL_SB2006, _abi.CMX_VEL_CHEN2022, 1 << 3, 1 << 31):              # CMX_SB2006_LIMITED is the only flag
        assert call(flags=bit) == BAD and call(flags=bit | _abi.CMX_SB2006_LIMITED) == BAD, hex(bit)
    bad_wr = P.WarmRainParams2M(ft, True)
    bad_wr.c.seifert_beheng.pdf_r.xr_min, bad_wr.c.seifert_beheng.pdf_r.xr_max = bad_wr.c.seifert_beheng.pdf_r.xr_max, bad_wr.c.seifert_beheng.pdf_r.xr_min
    assert call(w=bad_wr) == BAD                                                           # unordered limiter pair under CMX_SB2006_LIMITED


def test_python_wrapper_errors():
    wr, tps = P.WarmRainParams2M("f64", True), P.ThermodynamicsParameters("f64")
    cols = [torch.ones(4, dtype=torch.float64) for _ in range(7)]
    with pytest.raises(ValueError, match="unknown input 'rho'"):
        cmx.warm_rain_jacobian_2m(wr, tps, *cols, wrt=("T", "rho"))
    with pytest.raises(ValueError, match="unknown input"):
        cmx.warm_rain_jacobian_2m(wr, tps, *cols, wrt=("q_vap",))
    with pytest.raises(ValueError, match="listed twice"):
        cmx.warm_rain_jacobian_2m(wr, tps, *cols, wrt=("T", "T"))
    with pytest.raises(ValueError, match="nothing to compute"):
        cmx.warm_rain_jacobian_2m(wr, tps, *cols, wrt=())
    with pytest.raises(TypeError, match="mp must be"):
        cmx.warm_rain_jacobian_2m(object(), tps, *cols)
    with pytest.raises(ValueError, match="resident on the GPU"):          # there is no CPU path
        cmx.warm_rain_jacobian_2m(wr, tps, *cols)
    assert cmx.bulk_tendencies.JACOBIAN_WRT == _abi.SB2006_JAC_WRT == ("T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai")
    assert cmx.WarmRainJacobian2M._fields == ("jac", "tendencies", "wrt")
