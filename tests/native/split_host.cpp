// split_host.cpp — the alignment split of the streaming entry points (csrc/cmx_split.hpp) compiled by g++ for tests/test_split_host.py.
// The column addresses are plain numbers: the split only looks at them, it never dereferences one.
#include <cstdint>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_split.hpp"

extern "C" void split_host(const void *const *cols, int32_t ncols, int64_t n, int64_t elem, int32_t vec, int64_t *out) {
    const cmx::Split s = cmx::split_aligned(cols, ncols, n, (size_t)elem, vec);
    out[0] = s.head;
    out[1] = s.body;
    out[2] = s.tail;
}
