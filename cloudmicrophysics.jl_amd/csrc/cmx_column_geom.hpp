// cmx_column_geom.hpp — (column, level) of a flat point index, for the kernels that run one point per lane over columns stored level-fastest
// (the shells of cmx_column_products.hpp).
#pragma once
#include <cstdint>

#include "cmx_launch.hpp"

namespace cmx {

// (column, level) of flat index i = col·n_lev + lev
struct ColGeom {
    int64_t n;
    int32_t n_lev;
    double inv_n_lev;
    FastDivU32 lev_div;    // division by n_lev for flat indices below 2³² (cmx_launch.hpp fastdiv)
};
inline ColGeom make_col_geom(int64_t n, int32_t n_lev) { return {n, n_lev, 1.0 / (double)n_lev, make_fastdiv((uint32_t)n_lev)}; }
__device__ __forceinline__ void column_level(const ColGeom &g, int64_t i, int64_t &col, int32_t &lev) {
    if (g.n < ((int64_t)1 << 32)) {             // wave-uniform: one v_mul_hi_u32
        const uint32_t c32 = fastdiv((uint32_t)i, g.lev_div);
        col = c32;
        lev = (int32_t)((uint32_t)i - c32 * (uint32_t)g.n_lev);
    } else {                                    // one double multiply + fix-up per lane; exact below 2^53
        col = (int64_t)((double)i * g.inv_n_lev);
        int64_t k64 = i - col * g.n_lev;
        if (k64 < 0) { --col; k64 += g.n_lev; }
        if (k64 >= g.n_lev) { ++col; k64 -= g.n_lev; }
        lev = (int32_t)k64;
    }
}

}  // namespace cmx
