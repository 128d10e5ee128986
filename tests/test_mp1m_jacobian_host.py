"""The 1-moment tendency Jacobian without a GPU (include/cmx.h §(15), cmx.jacobian_1m):

  * the dual instantiation of the device point function (csrc/cmx_dual.hpp, csrc/cmx_mp1m_jacobian.hpp) compiled by g++ for the host
    (tests/native/derivatives_host.cpp) against central differences of the Float64 oracle — tests/jacobian_1m_cases.py has the states, the reference and
    the measure — at the reference's own bound 1e-5 (test/ad_compat_tests.jl:163) in Float64 and the project's Float32 bound 1e-3 in every row in Float32
    (worst Float32 row in this build: 1.5e-4, dq_icl_dt with the alternative options on the cold set);
  * the same parity in the second, input-scaled measure of tests/jacobian_cases.py (every entry weighted by |x_j|: it shows the T column, which the
    per-row scale hides behind the q columns) at the same two bounds: host build worst 9.7e-8 in Float64; 5.0e-4 in Float32 (dq_icl_dt × T, alternative
    options, cold set; every other entry ≤ 6.0e-5);
  * that both measures can fail: every input column scaled by 1.1, zeroed or negated is rejected, every entry reaches 1 % of its row in one of the
    measures on the cold and on the warm set, and every entry wrong by 0.2 % / 20 % is rejected;
  * the value parts against the plain instantiation, bit for bit; the columns against the tangent width K, bit for bit;
  * finiteness on every present / absent combination of the four species on both sides of T_freeze and on the broad synthetic set;
  * exact zeros from processes switched off by their option; the poison rules;
  * the argument statuses of the two entries and the Python wrapper's errors.

The host build proves the derivative RULES (its transcendentals are libm's, not the hardware's); tests/test_mp1m_jacobian_gpu.py repeats the parity
assertions on the device."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import jacobian_1m_cases as JC
import jacobian_host_build as JH
from jacobian_host_build import NPT, _same_bits, host_fixture
import cmx
from cmx import _abi, _lib, synthetic
from cmx import parameters as P

DT = {"f32": torch.float32, "f64": torch.float64}
T_FREEZE = 273.15
host = host_fixture()


def _head(ft, mp):
    return C.byref(mp.c), C.byref(P.ThermodynamicsParameters(ft)), C.c_uint32(mp.flags)


def host_jacobian(host, ft, mp, cols, wrt=JC.WRT, k=0, with_tendencies=True):
    """([4, len(wrt), n] Jacobian, [4, n] tendencies, status) of the host build; wrt: names in any order."""
    return JH.host_jacobian(host, "mp1m", ft, _head(ft, mp), cols, JC.WRT, wrt, k=k, with_tendencies=with_tendencies)


def host_plain(host, ft, mp, cols):
    return JH.host_plain(host, "mp1m", ft, _head(ft, mp), cols)


def _synthetic(ft):
    return [c.numpy() for c in synthetic.mp1m_state(4096, dtype=DT[ft], seed=1234)]


# ---- parity against the finite-difference reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("case", JC.CASES)
def test_host_jacobian_matches_central_differences_of_the_oracle(host, oracle, ft, case):
    """Float64: every row of every kept state within the reference's own 1e-5.  Float32, same Float64 reference: every row within 1e-3.  Both in the
    per-row and, every (row, column), in the input-scaled measure."""
    mp = JC.params(ft, case)
    for which in JC.SETS:
        J, _, rc = host_jacobian(host, ft, mp, JC.reference(case, which)[0])
        assert rc == (1 if case == "default" else 0)         # which instantiation ran: the one flags_1m selects
        JC.assert_parity(ft, J, case, which, "host")


# ---- the two measures can fail ------------------------------------------------------------------------------------------------------------------
MUTATIONS = (("scaled by 1.1", 1.1), ("zeroed", 0.0), ("negated", -1.0))


def _rejected(ft, M, case, which):
    try:
        JC.assert_parity(ft, M, case, which, "mutated", report=False)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("case", JC.CASES)
def test_a_corrupted_column_is_rejected(host, oracle, ft, case):
    """Each of the six input columns of the host-build Jacobian, whole, scaled by 1.1, zeroed or negated: assert_parity raises, in both float types, on
    every set.  (The row measure alone accepts the T column scaled by 1.1 in Float32: test_the_row_measure_alone_does_not_see_the_T_column.)"""
    mp = JC.params(ft, case)
    for which in JC.SETS:
        cols, J_ref, kept, _ = JC.reference(case, which)
        J, _, _ = host_jacobian(host, ft, mp, cols)
        assert not _rejected(ft, J, case, which)
        for j, name in enumerate(JC.WRT):
            assert np.any(J_ref[:, j, kept] != 0), name
            for kind, f in MUTATIONS:
                M = np.array(J)
                M[:, j] *= NPT[ft](f)
                assert _rejected(ft, M, case, which), (which, name, kind)


@pytest.mark.parametrize("case", JC.CASES)
def test_the_row_measure_alone_does_not_see_the_T_column(host, oracle, case):
    """Why the second measure exists: with the T column 10 % wrong at every state the per-row measure stays inside the FLOAT32 bound on both interior
    sets, the input-scaled one shows 0.1/1.1."""
    for which in ("cold", "warm"):
        cols, J_ref, kept, _ = JC.reference(case, which)
        J, _, _ = host_jacobian(host, "f64", JC.params("f64", case), cols)
        M = np.array(J)
        M[:, 0] *= 1.1
        assert max(JC.worst_rows(M, J_ref, kept, JC.OUT).values()) < JC.BOUND["f32"], which
        assert abs(JC.worst_cells(M, J_ref, cols[1:], kept).max() - 0.1 / 1.1) < 1e-6, which


@pytest.mark.parametrize("case", JC.CASES)
def test_every_entry_of_the_reference_is_resolved_by_the_interior_sets(host, oracle, case):
    """From the reference alone: all 24 entries are non-zero on the cold and on the warm set, and each reaches at least 1 % of its row in one of the two
    measures at some kept state (jacobian_cases.assert_resolution prints the relative error each entry is resolved to; the smallest share is 0.03,
    dq_sno_dt × (q_tot, q_lcl) on the warm sets).  Then the same with the code under test: every entry of the host-build Jacobian wrong by 0.2 % (Float64)
    or 20 % (Float32) at every state is rejected — twice the error the 1 % share promises to see."""
    for which in ("cold", "warm"):
        cols, J_ref, kept, _ = JC.reference(case, which)
        share, nonzero = JC.assert_resolution(J_ref, cols[1:], kept, JC.OUT, JC.WRT, f"1-moment {case} {which}")
        assert nonzero.all()
        for ft, f in (("f64", 1.002), ("f32", 1.2)):
            J, _, _ = host_jacobian(host, ft, JC.params(ft, case), cols)
            for i, j in zip(*np.nonzero(nonzero)):
                M = np.array(J)
                M[i, j] *= NPT[ft](f)
                assert _rejected(ft, M, case, which), (which, ft, JC.OUT[i], JC.WRT[j], float(share[i, j]))


def test_the_exponent_overrides_leave_the_default_exponent_instantiation(host, oracle):
    """The third parameter case is not mp1m_default_exponents: the run-time-flags instantiation runs and its tendencies differ from the default set's."""
    cols = JC.reference("exponents", "warm")[0]
    a, rca = host_plain(host, "f64", JC.params("f64", "default"), cols)
    b, rcb = host_plain(host, "f64", JC.params("f64", "exponents"), cols)
    assert (rca, rcb) == (1, 0)
    assert np.all(np.abs(a[2:] - b[2:]).max(axis=0) > 1e-6 * np.abs(a[2:]).max(axis=0))          # the rain and snow rows move at every state


# ---- the primal ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("case", JC.CASES)
def test_value_parts_are_the_plain_instantiation_bit_for_bit(host, oracle, ft, case):
    mp = JC.params(ft, case)
    for cols in (JC.reference(case, "cold")[0], JC.reference(case, "warm")[0], _synthetic(ft)):
        plain, rc = host_plain(host, ft, mp, cols)
        assert rc == (1 if case == "default" else 0)
        for wrt in (JC.WRT, ("q_rai",), ()):
            _, tend, _ = host_jacobian(host, ft, mp, cols, wrt=wrt)
            assert _same_bits(tend, plain), wrt


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("case", ["default", "alt"])
def test_columns_do_not_depend_on_the_tangent_width_or_the_selection(host, oracle, ft, case):
    """Each tangent is computed by the same operations whatever K is and whichever other inputs are seeded: K = 1, 2, 3, 6, subsets in any order."""
    mp = JC.params(ft, case)
    cols = [np.concatenate([a[:256], b[:256]]) for a, b in zip(JC.reference(case, "cold")[0], JC.reference(case, "warm")[0])]
    full, _, _ = host_jacobian(host, ft, mp, cols)
    for k in (1, 2, 3, 6):
        J, _, rc = host_jacobian(host, ft, mp, cols, k=k)
        assert rc in (0, 1) and _same_bits(J, full), k
    for wrt in (("q_sno", "T"), ("q_lcl",), ("q_rai", "q_tot", "q_icl", "T", "q_lcl")):
        J, _, _ = host_jacobian(host, ft, mp, cols, wrt=wrt)
        for kk, name in enumerate(wrt):
            assert _same_bits(J[:, kk], full[:, JC.WRT.index(name)]), (wrt, name)


# ---- finiteness ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("case", JC.CASES)
def test_jacobian_is_finite_with_absent_species(host, oracle, ft, case):
    """The 16 present / absent combinations of (q_lcl, q_icl, q_rai, q_sno) ∈ {0, interior value} at ρ = 1, 10 K below, at and 10 K above T_freeze, sub-
    and super-saturated: every entry is finite, and the column of an absent species is exactly zero — the input clamp max(0, x) passes no tangent at
    x = 0 and every gate behind it is a select or a floor."""
    states = []
    for T in (T_FREEZE - 10.0, T_FREEZE, T_FREEZE + 10.0):
        qs = float(JC.q_sat_liquid(oracle, np.array([T]), np.array([1.0]))[0])
        for sat in (0.7, 1.03):
            for present in itertools.product((0, 1), repeat=4):
                q = [v * p for v, p in zip((5e-4, 3e-4, 4e-4, 2e-4), present)]
                states.append((1.0, T, sum(q) + sat * qs, *q))
    cols = JC.points(*states)
    J, tend, _ = host_jacobian(host, ft, JC.params(ft, case), cols)
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(tend))
    for name in ("q_lcl", "q_icl", "q_rai", "q_sno"):
        j = JC.WRT.index(name)
        absent = cols[j + 1] == 0
        assert absent.sum() == 48 and np.all(J[:, j, absent] == 0), name


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("case", JC.CASES)
def test_jacobian_is_finite_wherever_the_tendencies_are(host, ft, case):
    """The broad synthetic set: exact zeros, slightly negative values, every gate, both sides of T_freeze."""
    J, tend, _ = host_jacobian(host, ft, JC.params(ft, case), _synthetic(ft))
    finite = np.isfinite(tend).all(axis=0)
    assert finite.sum() > 0.9 * finite.size
    assert np.all(np.isfinite(J[:, :, finite]))


@pytest.mark.parametrize("ft", ["f64", "f32"])
def test_a_process_switched_off_by_its_option_contributes_exact_zeros(host, oracle, ft):
    names = list(P.Microphysics1MOptions._defaults)
    off = {k: None for k in names}
    cols = [np.concatenate([a[:256], b[:256]]) for a, b in zip(JC.reference("default", "cold")[0], JC.reference("default", "warm")[0])]
    J, tend, rc = host_jacobian(host, ft, P.Microphysics1MParams(ft, **off), cols)              # nothing on: nothing but zeros
    assert rc == 0 and np.all(J == 0) and np.all(tend == 0)
    # one process on: only the rows it feeds are non-zero (row order dq_lcl, dq_icl, dq_rai, dq_sno)
    for on, rows in (("cloud_liquid_formation", (0,)), ("rain_condensation_evaporation", (2,)), ("snow_melt", (2, 3)), ("cloud_ice_snow_accretion", (1, 3)),
                     ("rain_autoconversion", (0, 2))):
        J, tend, _ = host_jacobian(host, ft, P.Microphysics1MParams(ft, **{k: v for k, v in off.items() if k != on}), cols)
        for o in range(4):
            if o in rows:
                assert np.any(J[o] != 0) and np.any(tend[o] != 0), (on, o)
            else:
                assert np.all(J[o] == 0) and np.all(tend[o] == 0), (on, o)
    # … and a process that is on but gated off contributes the same exact zeros: below freezing, snow melt switched off changes no bit (both calls run the
    # run-time-flags instantiation)
    cold = JC.reference("default", "cold")[0]
    a, ta, rca = host_jacobian(host, ft, P.Microphysics1MParams(ft, snow_melt=None, cloud_ice_melt=None), cold)
    b, tb, rcb = host_jacobian(host, ft, P.Microphysics1MParams(ft, cloud_ice_melt=None), cold)
    assert (rca, rcb) == (0, 0) and _same_bits(a, b) and _same_bits(ta, tb)


# ---- the poison rules ---------------------------------------------------------------------------------------------------------------------------
def test_a_nan_input_or_a_bad_density_poisons_every_output_of_its_point(host, oracle):
    for ft in ("f64", "f32"):
        mp = JC.params(ft, "default")
        cols = [np.array(c[:16], dtype=NPT[ft]) for c in JC.reference("default", "warm")[0]]
        clean, ctend, _ = host_jacobian(host, ft, mp, cols)
        keep = np.arange(16) != 5
        for j, v in [(j, np.nan) for j in range(7)] + ([(0, 0.0), (0, -1.0)] if ft == "f64" else []):
            bad = [c.copy() for c in cols]
            bad[j][5] = v
            J, tend, _ = host_jacobian(host, ft, mp, bad)
            assert np.all(np.isnan(J[:, :, 5])) and np.all(np.isnan(tend[:, 5])), (j, v)
            assert _same_bits(J[:, :, keep], clean[:, :, keep]) and _same_bits(tend[:, keep], ctend[:, keep])


# ---- statuses and the wrapper's errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_argument_statuses_without_gpu(ft):
    """Every call below returns before any HIP runtime call."""
    lib = _lib.lib()
    fn = getattr(lib, f"cmx_mp1m_jacobian_{ft}")
    BAD, UNS, OK = _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED, _abi.CMX_OK
    mp, tps = P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft)
    seven = [C.c_void_p(4096 + 64 * k) for k in range(7)]
    jac = (C.c_void_p * _abi.CMX_MP1M_JAC_NCOL)(*[8192 + 64 * k for k in range(_abi.CMX_MP1M_JAC_NCOL)])
    tend = (C.c_void_p * 4)(*[16384 + 64 * k for k in range(4)])
    nojac, notend = (C.c_void_p * _abi.CMX_MP1M_JAC_NCOL)(), (C.c_void_p * 4)()
    huge = 16 * 0x7fffffff + 1

    def call(flags=mp.flags, n=8, cols=seven, j=jac, t=tend, w=mp, th=tps):
        return fn(C.byref(w.c) if w is not None else None, C.byref(th) if th is not None else None, flags, n, *cols, j, t, None)
    assert call(w=None) == BAD and call(th=None) == BAD                                   # no parameters
    assert call(n=-1) == BAD and call(n=huge) == UNS and call(n=0) == OK                   # the count rule
    assert call(n=0, cols=[None] * 7, j=None, t=None) == OK                                # n = 0 returns before the columns matter …
    for pair in ((_abi.CMX_1M_CLOUD_ICE_FORMATION_CONST, _abi.CMX_1M_CLOUD_ICE_FORMATION_TDEP), (_abi.CMX_1M_RAIN_ACNV_KESSLER, _abi.CMX_1M_RAIN_ACNV_PRESCRIBED_ND),
                 (_abi.CMX_1M_SNOW_ACNV_NO_SUPERSAT, _abi.CMX_1M_SNOW_ACNV_WITH_SUPERSAT), (_abi.CMX_1M_SNOW_SUBLIMATION_ONLY, _abi.CMX_1M_SNOW_DEP_AND_SUBL)):
        assert call(flags=pair[0] | pair[1]) == BAD and call(flags=mp.flags | pair[0] | pair[1]) == BAD, pair      # both members of an exclusive pair
        assert call(flags=pair[0] | pair[1], n=0) == BAD                                   # … but not before the flags, like the tendencies entry
    assert call(flags=1 << 17) == BAD and call(flags=1 << 31) == BAD                       # an unknown bit
    for k in range(7):                                                                     # a NULL input column
        assert call(cols=seven[:k] + [None] + seven[k + 1:]) == BAD, k
    assert call(j=None, t=None) == BAD and call(j=nojac, t=None) == BAD and call(j=nojac, t=notend) == BAD and call(j=None, t=notend) == BAD    # no output


def test_python_wrapper_errors():
    mp, tps = P.Microphysics1MParams("f64"), P.ThermodynamicsParameters("f64")
    cols = [torch.ones(4, dtype=torch.float64) for _ in range(7)]
    with pytest.raises(ValueError, match="unknown input 'rho'"):
        cmx.jacobian_1m(mp, tps, *cols, wrt=("T", "rho"))
    with pytest.raises(ValueError, match="unknown input"):
        cmx.jacobian_1m(mp, tps, *cols, wrt=("n_lcl",))
    with pytest.raises(ValueError, match="listed twice"):
        cmx.jacobian_1m(mp, tps, *cols, wrt=("T", "T"))
    with pytest.raises(ValueError, match="nothing to compute"):
        cmx.jacobian_1m(mp, tps, *cols, wrt=())
    with pytest.raises(TypeError, match="mp must be"):
        cmx.jacobian_1m(object(), tps, *cols)
    with pytest.raises(ValueError, match="resident on the GPU"):          # there is no CPU path
        cmx.jacobian_1m(mp, tps, *cols)
    assert cmx.JACOBIAN_WRT_1M == _abi.MP1M_JAC_WRT == ("T", "q_tot", "q_lcl", "q_icl", "q_rai", "q_sno")
    assert cmx.JACOBIAN_OUTPUTS_1M == _abi.MP1M_JAC_OUT == ("dq_lcl_dt", "dq_icl_dt", "dq_rai_dt", "dq_sno_dt")
    assert cmx.Jacobian1M._fields == ("jac", "tendencies", "wrt")
