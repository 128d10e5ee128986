"""The Jacobian driver of csrc/cmx_jacobian.hpp is scheme-independent (no GPU): both real schemes are 4 × 6, so the slot table, the pass loop and the
stores are run here on the toy scheme of tests/native/derivatives_host.cpp — 3 outputs, 5 differentiated inputs, sums and products only.  On small-integer
states every value and derivative is exact in Float32 and Float64, so the analytic Jacobian is asserted with ==.  K = 1 … 5: SLOTS = ⌈5/K⌉·K pads the last
pass with idle slots for K = 2, 3, 4."""
import numpy as np
import pytest

import jacobian_host_build as JH
from jacobian_host_build import CT, NPT, _same_bits

host = JH.host_fixture()
WRT = ("a", "b", "c", "d", "e")
W = 2.0
SENTINEL = -777.0
BAD_ARG = -1      # CMX_ERR_BAD_ARG (include/cmx.h)


def states(n=37, seed=3):
    """(rho, a, b, c, d, e): integers in [-6, 6], zero included"""
    return [c.astype(np.float64) for c in np.random.default_rng(seed).integers(-6, 7, size=(6, n))]


def analytic(cols):
    r, a, b, c, d, e = cols
    one, zero = np.ones_like(r), np.zeros_like(r)
    tend = np.stack([r * a * b + c, c * d + W * e + a, a * b * c + d * e * r])
    jac = np.stack([np.stack([r * b, r * a, one, zero, zero]), np.stack([one, zero, d, c, W * one]), np.stack([b * c, a * c, a * b, e * r, d * r])])
    return jac, tend


def toy(host, ft, cols, wrt=WRT, k=0, with_tendencies=True, null=()):
    """null: (output, input name) members of the Jacobian left NULL."""
    jac, tend, rc = JH.host_jacobian(host, "toy", ft, (CT[ft](W),), cols, WRT, wrt, nout=3, k=k, with_tendencies=with_tendencies, sentinel=SENTINEL,
                                     null=null)
    return jac, tend, rc


@pytest.mark.parametrize("ft", ["f64", "f32"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_toy_jacobian_is_exact_at_every_tangent_width(host, ft, k):
    cols = states()
    J_ref, t_ref = analytic(cols)
    J, tend, passes = toy(host, ft, cols, k=k)
    assert passes == -(-5 // k)
    assert J.dtype == NPT[ft] and np.array_equal(J, J_ref) and np.array_equal(tend, t_ref)
    J1, t1, _ = toy(host, ft, cols, k=1)
    assert _same_bits(J, J1) and _same_bits(tend, t1)                    # columns independent of K
    # a subset in reversed order gives the columns of the full call
    for wrt in (("e", "c", "a"), ("d", "b"), WRT[::-1]):
        S, _, passes = toy(host, ft, cols, wrt=wrt, k=k, with_tendencies=False)
        assert passes == -(-len(wrt) // k)
        for kk, name in enumerate(wrt):
            assert _same_bits(S[:, kk], J[:, WRT.index(name)]), (wrt, name)
    # a NULL member leaves its sentinel, and only it
    null = ((1, "c"), (2, "e"), (0, "a"))
    N, tend, _ = toy(host, ft, cols, k=k, null=null)
    for o in range(3):
        for j, name in enumerate(WRT):
            assert np.all(N[o, j] == SENTINEL) if (o, name) in null else np.array_equal(N[o, j], J_ref[o, j]), (o, name)
    assert np.array_equal(tend, t_ref)
    # the tendencies-only call runs one pass; no output at all is an error
    E, tend, passes = toy(host, ft, cols, wrt=(), k=k)
    assert passes == 1 and E.shape == (3, 0, cols[0].size) and np.array_equal(tend, t_ref)
    assert toy(host, ft, cols, wrt=(), k=k, with_tendencies=False)[2] == BAD_ARG


def test_toy_default_width_and_unlisted_width(host):
    cols = states(5)
    assert toy(host, "f64", cols)[2] == 2                                 # k = 0: K = 3, two passes
    assert toy(host, "f64", cols, k=6)[2] == BAD_ARG and toy(host, "f32", cols, k=-1)[2] == BAD_ARG
