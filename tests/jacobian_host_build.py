"""What the host-build tests of the derivative layer share (tests/test_sb2006_jacobian_host.py, tests/test_mp1m_jacobian_host.py,
tests/test_jacobian_driver_host.py, tests/jacobian_products_cases.py): the fixture that compiles tests/native/derivatives_host.cpp with g++, the ctypes calls
into it, and bit-for-bit equality."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
NPT = {"f32": np.float32, "f64": np.float64}
CT = {"f32": C.c_float, "f64": C.c_double}


@functools.lru_cache(maxsize=None)
def _build(name):
    out = REPO / "tests" / "native" / "_build"
    out.mkdir(exist_ok=True)
    so = out / f"lib{name}.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(REPO / "tests" / "native" / f"{name}.cpp")], check=True)
    return C.CDLL(str(so))


def host_fixture(name="derivatives_host"):
    """A module-scoped fixture: tests/native/<name>.cpp built into tests/native/_build/lib<name>.so and loaded, once per process."""
    @pytest.fixture(scope="module")
    def host():
        return _build(name)
    return host


def _arr(ft, cols):
    return (C.POINTER(CT[ft]) * len(cols))(*[c.ctypes.data_as(C.POINTER(CT[ft])) if c is not None else None for c in cols])


JAC, JVP, VJP = 0, 1, 2


def host_call(host, entry, ft, what, head, k, cols, p, q, tend):
    """The status of host_<entry>_derivative_<ft>(what, *head, k, n, x, p, q, tend); what: JAC (p = None, q = the jac table), JVP (p = tangents, q = jvp) or VJP
    (p = cotangents, q = grad); head: the ctypes arguments in front of k (parameters and flags)."""
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    fn = getattr(host, f"host_{entry}_derivative_{ft}")
    fn.restype = C.c_int32
    return fn(C.c_int(what), *head, C.c_int(k), C.c_int64(x[0].size), _arr(ft, x), _arr(ft, p) if p is not None else None, _arr(ft, q) if q is not None else None,
              _arr(ft, list(tend)) if tend is not None else None)


def host_jacobian(host, entry, ft, head, cols, all_wrt, wrt, nout=4, k=0, with_tendencies=True, sentinel=np.nan, null=()):
    """([nout, len(wrt), n] Jacobian, [nout, n] tendencies, status) of host_call(…, JAC, …); all_wrt: the entry's differentiable inputs in ABI order; wrt: names
    in any order; null: (output, name) members left NULL.  Both results start as `sentinel`."""
    n = np.asarray(cols[0]).size
    jac = np.full((nout, len(wrt), n), sentinel, dtype=NPT[ft])
    tend = np.full((nout, n), sentinel, dtype=NPT[ft]) if with_tendencies else None
    slots = [None] * (nout * len(all_wrt))
    for kk, name in enumerate(wrt):
        for o in range(nout):
            if (o, name) not in null:
                slots[o * len(all_wrt) + all_wrt.index(name)] = jac[o, kk]
    return jac, tend, host_call(host, entry, ft, JAC, head, k, cols, None, slots, tend)


def host_plain(host, entry, ft, head, cols, nout=4):
    """([nout, n] tendencies, status) of host_<entry>_plain_<ft>(*head, n, x, y): the plain instantiation of the point function."""
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    y = np.empty((nout, x[0].size), dtype=NPT[ft])
    fn = getattr(host, f"host_{entry}_plain_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_int64(x[0].size), _arr(ft, x), _arr(ft, list(y)))
    return y, rc


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(np.all((a.view(np.uint8) == b.view(np.uint8)).reshape(a.shape + (-1,)).all(axis=-1) | (np.isnan(a) & np.isnan(b))))
