// cmx_split.hpp — the alignment split of the streaming entry points: host arithmetic only, no HIP (tests/native/split_host.cpp
// compiles it with g++).  cmx_launch.hpp for_each_range turns the split into launches.
#pragma once
#include <cstddef>
#include <cstdint>

namespace cmx {

// How n points of a set of columns are split into launches (include/cmx.h: any alignment is accepted and results are bit-identical
// whatever the alignment).  The vector body reads and writes `vec` points per lane, so every column must start it on an
// A = vec · elem byte boundary (16 B for f32x4 and f64x2, 8 B for the LinearizedAverage f32 pair).  That holds when every column sits at the
// same offset modulo A — as in any common slice [lo:hi] of aligned columns: `head` points are peeled up to the boundary, the body runs
// vec points per lane, and the ragged `tail` one point per lane.  NULL (absent optional) columns do not count.  If the columns'
// offsets differ, the first one is not even aligned to its element size, or vec = 1, everything is one scalar range: head = n.  Every
// instantiation computes the identical instruction sequence per point (-ffp-contract=off), so the split does not change any result.
struct Split { int64_t head, body, tail; };

inline Split split_aligned(const void *const *cols, int ncols, int64_t n, size_t elem, int vec) {
    const uintptr_t A = (uintptr_t)vec * elem;
    bool have = false, same = vec > 1;
    uintptr_t mis = 0;
    for (int k = 0; k < ncols && same; ++k) {
        if (!cols[k]) continue;
        const uintptr_t m = reinterpret_cast<uintptr_t>(cols[k]) % A;
        same = have ? m == mis : m % elem == 0;
        mis = m;
        have = true;
    }
    if (!same) return {n, 0, 0};
    const int64_t want = mis ? (int64_t)((A - mis) / elem) : 0;
    const int64_t head = want < n ? want : n;
    const int64_t body = (n - head) / vec * vec;
    return {head, body, n - head - body};
}

}  // namespace cmx
