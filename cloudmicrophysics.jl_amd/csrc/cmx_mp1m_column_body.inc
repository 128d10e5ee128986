// cmx_mp1m_column_body.inc — the body of the two 1-moment column kernels of cmx_mp1m_column.hip (mp1m_column_kernel: the fixed snow aspect ratio;
// mp1m_column_shaped_kernel: a snow shape), included INSIDE each kernel.  In the scope of the include: FT, FLAGS, LIN, GENERAL_GAMMA, VEC, BS,
// SHAPED and the kernel parameters a0, io, first, nvec.  Textual inclusion rather than an inlined device function keeps the instruction stream
// of mp1m_column_kernel byte for byte what it was before the shaped kernel existed (as a __forceinline__ function taking the kernel
// arguments by reference, the compiler schedules the kernel-argument loads differently).
// (no include guard: included once per kernel)
    using M = Math<FT>;
    const auto &a = CMX_MP1M_COL_CONSTS;
    __shared__ __align__(16) FT halo[BS + 1][4];   // fluxes of every lane's FIRST point, + slot BS for the point that follows the tile
    // tiles overlap by one lane, as in sb2006_column_kernel (cmx_sb2006_column.hip): lane BS−1 evaluates the next tile's first vector and only
    // supplies the flux its first point sends down; the flux-only evaluation of that point runs in the last workgroup of a launch only
    const int64_t tile0 = (int64_t)blockIdx.x * (BS - 1);
    const int64_t v = tile0 + threadIdx.x;
    const bool active = v < nvec;
    const int64_t nvalid = nvec - tile0 < BS ? nvec - tile0 : BS;       // active lanes of this tile (≥ 1)
    const bool owner = threadIdx.x < BS - 1;
    const int64_t i0 = first + v * VEC;                                 // flat index of the lane's first point

    FT x[7][VEC];
    if (active) {
#pragma unroll
        for (int j = 0; j < 7; ++j) load_col<FT, VEC, CMX_MP1M_COL_NT_IN>(io.in[j] + first, v, x[j]);
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS while the loads fly (every lane of the workgroup reaches the barrier inside); no-op for Float32
    if (nvalid < BS && threadIdx.x == BS - 1) {   // last workgroup of the launch: the point after its last vector, from the raw columns
        const int64_t e = first + (tile0 + nvalid) * VEC;
        SedFlux4<FT> f{{FT(0), FT(0), FT(0), FT(0)}};
        if (e < io.n) f = mp1m_sed_fluxes<FT, GENERAL_GAMMA, SHAPED>(a.vc, io.in[0][e], io.in[3][e], io.in[4][e], io.in[5][e], io.in[6][e]);
#pragma unroll
        for (int s = 0; s < 4; ++s) halo[BS][s] = f.f[s];
    }
    // per point: A = tendency − (own flux)·g (final but for the inflow), g = 1/(ρ Δz)
    FT A[VEC][4], g[VEC];
    SedFlux4<FT> F[VEC];
    int64_t col = 0;
    int32_t lev = 0;
    if (active) {
        if (io.n < ((int64_t)1 << 32)) {                  // i0 = col·n_lev + k; wave-uniform: one v_mul_hi_u32 (cmx_launch.hpp fastdiv)
            const uint32_t c32 = fastdiv((uint32_t)i0, io.lev_div);
            col = c32;
            lev = (int32_t)((uint32_t)i0 - c32 * (uint32_t)io.n_lev);
        } else {                                          // one double multiply + fix-up per lane; exact below 2^53
            col = (int64_t)((double)i0 * io.inv_n_lev);
            int64_t k64 = i0 - col * io.n_lev;
            if (k64 < 0) { --col; k64 += io.n_lev; }
            if (k64 >= io.n_lev) { ++col; k64 -= io.n_lev; }
            lev = (int32_t)k64;
        }
        int32_t lv = lev;
        const auto &k = a.k;
        // two passes over the lane's points — tendencies, then fluxes — so that only one pass's constants are live at a time
        FT t[VEC][4];
        // one value of the value type VT at a time: a point, or — Float32 with four points per lane — a PAIR of points in packed arithmetic (cmx_math.hpp f32x2;
        // not the run-time-Γ instantiation: an OCML call per lane, nothing to pack)
        constexpr int L = (sizeof(FT) == 4 && VEC % 2 == 0 && !GENERAL_GAMMA) ? 2 : 1;
        using VT = std::conditional_t<L == 2, f32x2, FT>;
        using MV = Math<VT>;
        if constexpr (L == 1) {      // (kept verbatim from rounds 3–4: routing the one-point case through the generic form below doubled its registers)
#pragma unroll
            for (int p = 0; p < VEC; ++p) {
                if constexpr (LIN)
                    mp1m_linearized_point<FT, FLAGS>(k.c, [&](FT dep) -> decltype(auto) { return CMX_MP1M_COL_LIN_ARGS(k, dep); }, CMX_MP1M_COL_NSUB, x[0][p], x[1][p], x[2][p],
                                                     x[3][p], x[4][p], x[5][p], x[6][p], t[p][0], t[p][1], t[p][2], t[p][3]);
                else
                    mp1m_tendencies_point<FT, FLAGS>(k.c, x[0][p], x[1][p], x[2][p], x[3][p], x[4][p], x[5][p], x[6][p], t[p][0], t[p][1], t[p][2], t[p][3]);
            }
            const auto &vc = consts_after(a, t[VEC - 1][3]).vc;
#pragma unroll
            for (int p = 0; p < VEC; ++p) {
                F[p] = mp1m_sed_fluxes<FT, GENERAL_GAMMA, SHAPED>(vc, x[0][p], x[3][p], x[4][p], x[5][p], x[6][p]);
                g[p] = io.inv_dz[lv] * M::rcp(max0(x[0][p]));                          // 1/(ρ_k Δz_k)
                if (++lv == io.n_lev) lv = 0;
#pragma unroll
                for (int s = 0; s < 4; ++s) A[p][s] = M::fma(-F[p].f[s], g[p], t[p][s]);
            }
        } else {
            auto val = [&x](int j, int p) -> VT {
                if constexpr (L == 2) return VT{x[j][p], x[j][p + 1]};
                else return x[j][p];
            };
#pragma unroll
            for (int p = 0; p < VEC; p += L) {
                VT tt[4];
                if constexpr (LIN)
                    mp1m_linearized_point<VT, FLAGS>(k.c, [&](VT dep) -> decltype(auto) { return CMX_MP1M_COL_LIN_ARGS(k, dep); }, CMX_MP1M_COL_NSUB, val(0, p), val(1, p), val(2, p),
                                                     val(3, p), val(4, p), val(5, p), val(6, p), tt[0], tt[1], tt[2], tt[3]);
                else
                    mp1m_tendencies_point<VT, FLAGS>(k.c, val(0, p), val(1, p), val(2, p), val(3, p), val(4, p), val(5, p), val(6, p), tt[0], tt[1], tt[2], tt[3]);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if constexpr (L == 2) { t[p][s] = tt[s].x; t[p + 1][s] = tt[s].y; }
                    else t[p][s] = tt[s];
                }
            }
            const auto &vc = consts_after(a, t[VEC - 1][3]).vc;
#pragma unroll
            for (int p = 0; p < VEC; p += L) {
                const SedFlux4<VT> Fp = mp1m_sed_fluxes<VT, GENERAL_GAMMA, SHAPED>(vc, val(0, p), val(3, p), val(4, p), val(5, p), val(6, p));
                VT gp;                                                                 // 1/(ρ_k Δz_k)
                if constexpr (L == 2) {
                    const FT dz0 = io.inv_dz[lv];
                    if (++lv == io.n_lev) lv = 0;
                    const FT dz1 = io.inv_dz[lv];
                    if (++lv == io.n_lev) lv = 0;
                    gp = VT{dz0, dz1} * MV::rcp(max0(val(0, p)));
                } else {
                    gp = io.inv_dz[lv] * MV::rcp(max0(val(0, p)));
                    if (++lv == io.n_lev) lv = 0;
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    VT tt;
                    if constexpr (L == 2) tt = VT{t[p][s], t[p + 1][s]};
                    else tt = t[p][s];
                    const VT As = MV::fma(-Fp.f[s], gp, tt);
                    if constexpr (L == 2) { A[p][s] = As.x; A[p + 1][s] = As.y; F[p].f[s] = Fp.f[s].x; F[p + 1].f[s] = Fp.f[s].y; }
                    else { A[p][s] = As; F[p].f[s] = Fp.f[s]; }
                }
                if constexpr (L == 2) { g[p] = gp.x; g[p + 1] = gp.y; }
                else g[p] = gp;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) halo[threadIdx.x][s] = F[0].f[s];
    }
    __syncthreads();
    if (!active || !owner) return;
    const int up = (threadIdx.x + 1 < nvalid) ? threadIdx.x + 1 : BS;
    FT o[4][VEC];
#pragma unroll
    for (int p = 0; p < VEC; ++p) {
        const bool top = lev == io.n_lev - 1;       // nothing enters through the model top
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const FT upf = (p + 1 < VEC) ? F[p + 1 < VEC ? p + 1 : 0].f[s] : halo[up][s];
            o[s][p] = M::fma(top ? FT(0) : upf, g[p], A[p][s]);      // a select, not a branch per species
        }
        if (lev == 0) {                             // surface precipitation fluxes of the column
            if (io.precip_rai) io.precip_rai[col] = F[p].f[2];
            if (io.precip_sno) io.precip_sno[col] = F[p].f[3];
        }
        if (++lev == io.n_lev) { lev = 0; ++col; }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) store_col<FT, VEC, true>(io.out[s] + first, v, o[s]);
