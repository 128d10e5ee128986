"""CPU check of the rule every entry point picks its kernel instantiation by (csrc/cmx_dispatch.hpp dispatch / dispatch_or, through
tests/native/dispatch_host.cpp): run-time flags and modes become compile-time tags of ONE call of a generic lambda.  For one, two and
three selectors every combination of listed values calls the lambda exactly once with exactly those tags; a value that is not listed
calls it not at all and is reported; a status the lambda returns comes back unchanged."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
NONE = -99                        # a tag slot the case does not use (dispatch_host.cpp Record)
FLAG = (0, 1)
# case number of dispatch_host.cpp → the listed values of each selector, in the selectors' order (flags and one_of mixed both ways)
CASES = {
    0: (FLAG,),
    1: ((3, 5, 9),),
    2: (FLAG, (0, 1, 2, 3)),
    3: ((1, 2, 4), FLAG),
    4: (FLAG, (10, 20, 30), FLAG),
    5: ((1, 2), (7, 8, 9), (-1, 0)),
}
UNLISTED = (-2, 6, 11, 31, 1 << 20)    # in none of the one_of lists above


@pytest.fixture(scope="module")
def dispatch():
    out = REPO / "tests" / "native" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libdispatch_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", "-o", str(so), str(REPO / "tests" / "native" / "dispatch_host.cpp")],
                   check=True)
    lib = C.CDLL(str(so))
    lib.dispatch_host.restype = None
    lib.dispatch_host.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]

    def call(which, values, miss=0):
        v = list(values) + [0] * (3 - len(values))
        r = (C.c_int32 * 5)()
        lib.dispatch_host(which, v[0], v[1], v[2], miss, r)
        return {"calls": r[0], "tags": tuple(r[1:4]), "ret": r[4]}
    return call


def _pad(values):
    return tuple(values) + (NONE,) * (3 - len(values))


@pytest.mark.parametrize("which", sorted(CASES))
def test_every_listed_combination_calls_once_with_its_tags(dispatch, which):
    lists = CASES[which]
    combos = list(itertools.product(*lists))
    assert len(combos) == len(set(combos))
    for values in combos:
        got = dispatch(which, values)
        assert got == {"calls": 1, "tags": _pad(values), "ret": 1}, f"case {which} values {values}"


@pytest.mark.parametrize("which", [w for w in sorted(CASES) if any(lst is not FLAG for lst in CASES[w])])
def test_unlisted_value_calls_nothing_and_is_reported(dispatch, which):
    lists = CASES[which]
    for pos, lst in enumerate(lists):
        if lst is FLAG:
            continue      # a flag has no unlisted value
        for bad in UNLISTED:
            assert bad not in lst
            for values in itertools.product(*[(bad,) if k == pos else l for k, l in enumerate(lists)]):
                got = dispatch(which, values)
                assert got == {"calls": 0, "tags": _pad(()), "ret": 0}, f"case {which} values {values}"


def test_unsigned_values_beyond_int(dispatch):
    assert dispatch(6, (0x4003,)) == {"calls": 1, "tags": _pad((0,)), "ret": 1}
    assert dispatch(6, (0xFFFFFFFF,)) == {"calls": 1, "tags": _pad((1,)), "ret": 1}
    assert dispatch(6, (0x4002,)) == {"calls": 0, "tags": _pad(()), "ret": 0}


@pytest.mark.parametrize("miss", [-7, 0, 3])
def test_returned_status_comes_back_unchanged(dispatch, miss):
    for a, b, c in itertools.product(FLAG, (10, 20, 30), FLAG):
        got = dispatch(7, (a, b, c), miss)
        assert got == {"calls": 1, "tags": (a, b, c), "ret": 1000 + 100 * a + b + c}
    for a, b, c in itertools.product(FLAG, UNLISTED, FLAG):
        assert dispatch(7, (a, b, c), miss) == {"calls": 0, "tags": _pad(()), "ret": miss}


def test_excluded_combination_stays_inside_the_lambda(dispatch):
    """A listed value whose instantiation must not exist is an `if constexpr` in the lambda: it is called, and returns its own status."""
    assert dispatch(8, (3,), -7) == {"calls": 1, "tags": _pad((3,)), "ret": 0}
    assert dispatch(8, (5,), -7) == {"calls": 1, "tags": _pad((5,)), "ret": 0}
    assert dispatch(8, (9,), -7) == {"calls": 0, "tags": _pad(()), "ret": -9}
    assert dispatch(8, (4,), -7) == {"calls": 0, "tags": _pad(()), "ret": -7}
