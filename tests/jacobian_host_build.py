"""What the host-build Jacobian tests share (tests/test_sb2006_jacobian_host.py, tests/test_mp1m_jacobian_host.py, tests/test_jacobian_driver_host.py): the
fixture that compiles one of tests/native/*_host.cpp with g++, the ctypes calls into it, and bit-for-bit equality."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
NPT = {"f32": np.float32, "f64": np.float64}
CT = {"f32": C.c_float, "f64": C.c_double}


def host_fixture(name):
    """A module-scoped fixture: tests/native/<name>.cpp built into tests/native/_build/lib<name>.so and loaded."""
    @pytest.fixture(scope="module")
    def host():
        out = REPO / "tests" / "native" / "_build"
        out.mkdir(exist_ok=True)
        so = out / f"lib{name}.so"
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(REPO / "tests" / "native" / f"{name}.cpp")],
                       check=True)
        return C.CDLL(str(so))
    return host


def _arr(ft, cols):
    return (C.POINTER(CT[ft]) * len(cols))(*[c.ctypes.data_as(C.POINTER(CT[ft])) if c is not None else None for c in cols])


def host_jacobian(host, entry, ft, head, cols, all_wrt, wrt, nout=4, k=0, with_tendencies=True, sentinel=np.nan, null=()):
    """([nout, len(wrt), n] Jacobian, [nout, n] tendencies, status) of host_<entry>_<ft>(*head, k, n, x, jac, tend); head: the ctypes arguments in front of
    k (parameters and flags); all_wrt: the entry's differentiable inputs in ABI order; wrt: names in any order; null: (output, name) members left NULL.  Both results start as `sentinel`."""
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    n = x[0].size
    jac = np.full((nout, len(wrt), n), sentinel, dtype=NPT[ft])
    tend = np.full((nout, n), sentinel, dtype=NPT[ft]) if with_tendencies else None
    slots = [None] * (nout * len(all_wrt))
    for kk, name in enumerate(wrt):
        for o in range(nout):
            if (o, name) not in null:
                slots[o * len(all_wrt) + all_wrt.index(name)] = jac[o, kk]
    fn = getattr(host, f"host_{entry}_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_int(k), C.c_int64(n), _arr(ft, x), _arr(ft, slots), _arr(ft, list(tend)) if tend is not None else None)
    return jac, tend, rc


def host_plain(host, entry, ft, head, cols, nout=4):
    """([nout, n] tendencies, status) of host_<entry>_<ft>(*head, n, x, y): the plain instantiation of the point function."""
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    y = np.empty((nout, x[0].size), dtype=NPT[ft])
    fn = getattr(host, f"host_{entry}_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_int64(x[0].size), _arr(ft, x), _arr(ft, list(y)))
    return y, rc


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(np.all((a.view(np.uint8) == b.view(np.uint8)).reshape(a.shape + (-1,)).all(axis=-1) | (np.isnan(a) & np.isnan(b))))
