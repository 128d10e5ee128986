"""CPU check of the alignment split every streaming entry point launches by (csrc/cmx_split.hpp split_aligned, through
tests/native/split_host.cpp): scalar head, vector body, scalar tail, or one scalar range.  The column addresses are numbers that are
never dereferenced; the -m gpu suite checks that the launches built on the split give the same bits for any alignment."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
BASE = 0x7F3A_0000_0000          # a 4 KiB-aligned stand-in for a device allocation
K_MAX_POINTS = 16 * 0x7FFFFFFF   # cmx_launch.hpp kMaxPoints
SIZES = list(range(65)) + [1000, 1 << 20, 100_000_003, K_MAX_POINTS - 1, K_MAX_POINTS]
# (alignment A in bytes, element size): VEC = A / element size — f32x4 and f64x2 (16 B), the LinearizedAverage f32 pair (8 B), Float64 one
# point per lane (8 B, VEC = 1)
CASES = [(16, 4), (16, 8), (8, 4), (8, 8)]


@pytest.fixture(scope="module")
def split():
    out = REPO / "tests" / "native" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libsplit_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", "-o", str(so), str(REPO / "tests" / "native" / "split_host.cpp")],
                   check=True)
    lib = C.CDLL(str(so))
    lib.split_host.restype = None
    lib.split_host.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]

    def call(addrs, n, elem, vec):
        cols = (C.c_void_p * len(addrs))(*addrs)
        r = (C.c_int64 * 3)()
        lib.split_host(cols, len(addrs), n, elem, vec, r)
        return tuple(r)
    return call


def _old_formula(addrs, n, elem, vec):
    """What each entry point computed by hand before the split had one home: (head, body, tail), or None for one scalar range."""
    a = vec * elem
    live = [p for p in addrs if p is not None]
    mis0 = live[0] % a
    if vec == 1 or mis0 % elem or any(p % a != mis0 for p in live):
        return None
    head = min(n, (a - mis0) // elem if mis0 else 0)
    body = (n - head) // vec * vec
    return head, body, n - head - body


def _column_sets(a, off):
    """Column address lists whose first column sits `off` bytes past an A-byte boundary."""
    first = BASE + off
    yield [first], True
    yield [first, BASE + 3 * a + off], True                       # second column at the same offset
    yield [first, None, BASE + 5 * a + off], True                 # an absent optional column does not count
    yield [None, first, BASE + 7 * a + off], True                 # … not even in front
    for d in range(1, a):
        yield [first, BASE + 3 * a + (off + d) % a], False        # second column at another offset


@pytest.mark.parametrize("a,elem", CASES)
def test_split_covers_aligns_and_matches_the_old_formula(split, a, elem):
    vec = a // elem
    for off in range(a):
        for addrs, same in _column_sets(a, off):
            split_ok = same and vec > 1 and off % elem == 0
            for n in SIZES:
                head, body, tail = got = split(addrs, n, elem, vec)
                what = f"A={a} elem={elem} addrs={[None if p is None else p - BASE for p in addrs]} n={n}"
                assert min(got) >= 0 and head + body + tail == n, what            # contiguous, exactly [0, n)
                if not split_ok:
                    assert got == (n, 0, 0), what                                  # one scalar range
                    assert _old_formula(addrs, n, elem, vec) is None, what
                    continue
                assert body % vec == 0 and head < vec and tail < vec, what
                if body:
                    for p in addrs:
                        if p is not None:
                            assert (p + head * elem) % a == 0, what              # the body starts on an A-byte boundary in every column
                assert got == _old_formula(addrs, n, elem, vec), what


def test_linearized_pair_split_matches_its_old_rule(split):
    """The 1-moment LinearizedAverage f32 pair path had its own rule: peel one point if the columns sit 4 bytes off 8, pairs if n ≥ 2."""
    for off in (0, 4):
        for n in range(65):
            head, body, tail = split([BASE + off, BASE + 64 + off], n, 4, 2)
            old_head = (1 if off else 0) if n >= 2 else 0
            old_pairs = (n - old_head) // 2 if n >= 2 else 0
            # below two points the old rule ran one scalar range: the same single point-kernel launch as a head or tail of one point
            if n < 2:
                assert body == 0 and head + tail == n
            else:
                assert (head, body, tail) == (old_head, 2 * old_pairs, n - old_head - 2 * old_pairs)
