// cmx_sb2006_column_body.inc — the body of sb2006_column_kernel (cmx_sb2006_column.hip has the story), as text: the ensemble kernel
// (cmx_sb2006_ensemble.hip) includes the same lines, so both forms are the same operations on the same operands.  The including kernel provides
//   FT, LIMITED, VEL, CLOUD, VEC, BS, INTPOW     the template parameters of sb2006_column_kernel
//   cv, io, first, nvec                           CloudVelConsts<FT>, SbColIO<FT> of ONE set of columns (the point at index io.n does not exist and is never
//                                                 read), the flat index of the first vector and the number of vectors that blockIdx.x tiles
//   CMX_SB_COL_CONSTS(ALSO)                       the constants: an expression the point function takes as its first argument
//   CMX_SB_COL_NT_IN                              whether the vector loads of the state carry the non-temporal hint
    using M = Math<FT>;
    // fluxes of every lane's FIRST point, + slot BS for the point that follows the tile
    __shared__ __align__(16) FT halo[BS + 1][4];
    // Tiles OVERLAP by one lane (round 4): workgroup b owns the vectors [b(BS−1), (b+1)(BS−1)); its lane BS−1 evaluates the first vector of the
    // next tile like any other lane and only supplies the flux its first point sends down to lane BS−2.  The redundant work is 1/(BS−1) of the
    // launch; evaluating that one point on its own (rounds 2–3) made the last wave of every workgroup issue the whole flux function once
    // more with one lane active — 12 of the Float32 kernel's 302 instructions per point (PMC).  Only the LAST workgroup of a launch, whose
    // last owned vector is followed by another launch's (or no) point, still takes that path.
    const int64_t tile0 = (int64_t)blockIdx.x * (BS - 1);
    const int64_t v = tile0 + threadIdx.x;
    const bool active = v < nvec;
    const int64_t nvalid = nvec - tile0 < BS ? nvec - tile0 : BS;       // active lanes of this tile (≥ 1)
    const bool owner = threadIdx.x < BS - 1;                            // lane BS−1 never stores: its vector belongs to the next workgroup
    const int64_t i0 = first + v * VEC;                                 // flat index of the lane's first point

    // all global loads first: the lane's seven 16-byte vectors, and (last lane only) the five scalars of the point after the tile
    FT rho[VEC], T[VEC], q_tot[VEC], q_lcl[VEC], n_lcl[VEC], q_rai[VEC], n_rai[VEC];
    if (active) {
        load_col<FT, VEC, CMX_SB_COL_NT_IN>(io.rho + first, v, rho);
        load_col<FT, VEC, CMX_SB_COL_NT_IN>(io.T + first, v, T);
        load_col<FT, VEC, CMX_SB_COL_NT_IN>(io.q_tot + first, v, q_tot);
        load_col<FT, VEC, CMX_SB_COL_NT_IN>(io.q_lcl + first, v, q_lcl);
        load_col<FT, VEC, CMX_SB_COL_NT_IN>(io.n_lcl + first, v, n_lcl);
        load_col<FT, VEC, CMX_SB_COL_NT_IN>(io.q_rai + first, v, q_rai);
        load_col<FT, VEC, CMX_SB_COL_NT_IN>(io.n_rai + first, v, n_rai);
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS while the loads fly (every lane of the workgroup reaches the barrier inside); no-op for Float32
    // the point after the tile (another workgroup's, or another launch's, first point) is evaluated here from the raw columns —
    // before the lane's own points, while nothing else is live in registers
    if (nvalid < BS && threadIdx.x == BS - 1) {        // last workgroup of the launch only (lane BS−1 has no vector there)
        const int64_t e = first + (tile0 + nvalid) * VEC;
        SedFlux<FT> f{FT(0), FT(0), FT(0), FT(0)};
        if (e < io.n) f = sed_fluxes_of_point<FT, LIMITED, VEL, CLOUD>(CMX_SB_COL_CONSTS(false), cv, io.rho[e], io.q_lcl[e], io.n_lcl[e], io.q_rai[e], io.n_rai[e]);
        halo[BS][0] = f.q_rai;
        halo[BS][1] = f.n_rai;
        halo[BS][2] = f.q_lcl;
        halo[BS][3] = f.n_lcl;
    }
    // per point: A = tendency − (own flux)·g (final but for the inflow), g = 1/(ρ Δz) and the flux the cell below receives
    FT A[VEC][4], g[VEC];
    SedFlux<FT> F[VEC];
    int64_t col = 0;
    int32_t lev = 0;
    if (active) {
        // level of the lane's first point: i0 = col·n_lev + k
        if (io.n < ((int64_t)1 << 32)) {             // wave-uniform: one v_mul_hi_u32 (≈ 7 instructions against ≈ 40 of the Float64 quotient)
            const uint32_t c32 = fastdiv((uint32_t)i0, io.lev_div);
            col = c32;
            lev = (int32_t)((uint32_t)i0 - c32 * (uint32_t)io.n_lev);
        } else {                                     // one double multiply + fix-up per lane; exact below 2^53
            col = (int64_t)((double)i0 * io.inv_n_lev);
            int64_t k64 = i0 - col * io.n_lev;
            if (k64 < 0) { --col; k64 += io.n_lev; }
            if (k64 >= io.n_lev) { ++col; k64 -= io.n_lev; }
            lev = (int32_t)k64;
        }
        int32_t lv = lev;
        // one value of the value type VT at a time: a point, or — Float32 with four points per lane — a PAIR of points in packed arithmetic (cmx_math.hpp f32x2)
        constexpr int L = (sizeof(FT) == 4 && VEC % 2 == 0 && VEL != VEL_CHEN_GEN) ? 2 : 1;    // (the run-time Γ of the general Chen instantiation is an OCML call per lane: nothing to pack, 100 spilled VGPRs)
        if constexpr (L == 1) {      // one point at a time — rounds 2–4 verbatim (see sb2006_tendencies_kernel)
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                // clamp_to_nonneg — BMT:828-837 (T is not clamped)
                const FT r_ = max0(rho[k]), qt = max0(q_tot[k]), ql = max0(q_lcl[k]);
                const FT qr = max0(q_rai[k]), nl = max0(n_lcl[k]), nr = max0(n_rai[k]);
                const bool poisoned = any_nan(rho[k], q_tot[k], q_lcl[k], n_lcl[k], q_rai[k], n_rai[k], T[k]);
                const SbRates<FT> p = sb2006_point<FT, LIMITED, VEL, false, INTPOW>(CMX_SB_COL_CONSTS(false), r_, T[k], qt, ql, qr, r_ * nl, r_ * nr, nl, nr);
                F[k] = sed_fluxes<FT, CLOUD>(cv, r_, ql, nl, qr, nr, p.vt_n, p.vt_m);
                g[k] = io.inv_dz[lv] * p.inv_rho;                                  // 1/(ρ_k Δz_k)
                if (++lv == io.n_lev) lv = 0;
                // sums of warm_rain_tendencies_2m — BMT:738-779 (as in sb2006_tendencies_kernel), minus the outflow through the lower face
                A[k][0] = (p.cond + p.au_dq_lcl) + p.ac_dq_lcl;
                A[k][1] = M::fma(p.lsc_plus_au + p.ac_dN_lcl, p.inv_rho, p.na_lcl);
                A[k][2] = M::fma(-F[k].q_rai, g[k], (p.evq + p.au_dq_rai) + p.ac_dq_rai);
                A[k][3] = M::fma(-F[k].n_rai, g[k], M::fma(((p.evN + p.au_dN_rai) + p.rsc) + p.rbr, p.inv_rho, p.na_rai));
                if constexpr (CLOUD) {
                    A[k][0] = M::fma(-F[k].q_lcl, g[k], A[k][0]);
                    A[k][1] = M::fma(-F[k].n_lcl, g[k], A[k][1]);
                }
                // NaN rule (one rule for every path — ADVICE r02): a NaN in ANY input poisons the point's four tendencies; the FLUXES depend on
                // (ρ, q_lcl, n_lcl, q_rai, n_rai) only — exactly the operands of sed_fluxes_of_point, which evaluates the point after the tile —
                // so a NaN in T or q_tot does not reach the cell below, wherever the tile boundary falls
                if (poisoned) A[k][0] = A[k][1] = A[k][2] = A[k][3] = M::nan();
                if (any_nan(rho[k], q_lcl[k], n_lcl[k], q_rai[k], n_rai[k])) F[k].q_rai = F[k].n_rai = F[k].q_lcl = F[k].n_lcl = M::nan();
            }
        } else {
            using VT = std::conditional_t<L == 2, f32x2, FT>;
            using MV = Math<VT>;
#pragma unroll
            for (int k = 0; k < VEC; k += L) {
                auto val = [k](const FT (&a)[VEC]) -> VT {
                    if constexpr (L == 2) return VT{a[k], a[k + 1]};
                    else return a[k];
                };
                const VT rho_k = val(rho), T_k = val(T), qt_k = val(q_tot), ql_k = val(q_lcl), nl_k = val(n_lcl), qr_k = val(q_rai), nr_k = val(n_rai);
                // clamp_to_nonneg — BMT:828-837 (T is not clamped)
                const VT r_ = max0(rho_k), qt = max0(qt_k), ql = max0(ql_k);
                const VT qr = max0(qr_k), nl = max0(nl_k), nr = max0(nr_k);
                const typename MV::Mask poisoned = nan_mask(rho_k, qt_k, ql_k, nl_k, qr_k, nr_k, T_k);
                const SbRates<VT> p = sb2006_point<VT, LIMITED, VEL, false, INTPOW>(CMX_SB_COL_CONSTS((L == 2)), r_, T_k, qt, ql, qr, r_ * nl, r_ * nr, nl, nr);
                SedFlux<VT> Fk = sed_fluxes<VT, CLOUD>(cv, r_, ql, nl, qr, nr, p.vt_n, p.vt_m);
                VT gk;                                                             // 1/(ρ_k Δz_k)
                if constexpr (L == 2) {
                    const FT dz0 = io.inv_dz[lv];
                    if (++lv == io.n_lev) lv = 0;
                    const FT dz1 = io.inv_dz[lv];
                    if (++lv == io.n_lev) lv = 0;
                    gk = VT{dz0, dz1} * p.inv_rho;
                } else {
                    gk = io.inv_dz[lv] * p.inv_rho;
                    if (++lv == io.n_lev) lv = 0;
                }
                // sums of warm_rain_tendencies_2m — BMT:738-779 (as in sb2006_tendencies_kernel), minus the outflow through the lower face
                VT Ak[4];
                Ak[0] = (p.cond + p.au_dq_lcl) + p.ac_dq_lcl;
                Ak[1] = MV::fma(p.lsc_plus_au + p.ac_dN_lcl, p.inv_rho, p.na_lcl);
                Ak[2] = MV::fma(-Fk.q_rai, gk, (p.evq + p.au_dq_rai) + p.ac_dq_rai);
                Ak[3] = MV::fma(-Fk.n_rai, gk, MV::fma(((p.evN + p.au_dN_rai) + p.rsc) + p.rbr, p.inv_rho, p.na_rai));
                if constexpr (CLOUD) {
                    Ak[0] = MV::fma(-Fk.q_lcl, gk, Ak[0]);
                    Ak[1] = MV::fma(-Fk.n_lcl, gk, Ak[1]);
                }
                // NaN rule (one rule for every path — ADVICE r02): a NaN in ANY input poisons the point's four tendencies; the FLUXES depend on
                // (ρ, q_lcl, n_lcl, q_rai, n_rai) only — exactly the operands of sed_fluxes_of_point, which evaluates the point after the tile —
                // so a NaN in T or q_tot does not reach the cell below, wherever the tile boundary falls
#pragma unroll
                for (int q = 0; q < 4; ++q) Ak[q] = poisoned ? MV::nan() : Ak[q];
                const typename MV::Mask fpoison = nan_mask(rho_k, ql_k, nl_k, qr_k, nr_k);
                Fk.q_rai = fpoison ? MV::nan() : Fk.q_rai; Fk.n_rai = fpoison ? MV::nan() : Fk.n_rai;
                Fk.q_lcl = fpoison ? MV::nan() : Fk.q_lcl; Fk.n_lcl = fpoison ? MV::nan() : Fk.n_lcl;
                if constexpr (L == 2) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { A[k][q] = Ak[q].x; A[k + 1][q] = Ak[q].y; }
                    g[k] = gk.x; g[k + 1] = gk.y;
                    F[k] = SedFlux<FT>{Fk.q_rai.x, Fk.n_rai.x, Fk.q_lcl.x, Fk.n_lcl.x};
                    F[k + 1] = SedFlux<FT>{Fk.q_rai.y, Fk.n_rai.y, Fk.q_lcl.y, Fk.n_lcl.y};
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) A[k][q] = Ak[q];
                    g[k] = gk;
                    F[k] = Fk;
                }
            }
        }
        halo[threadIdx.x][0] = F[0].q_rai;
        halo[threadIdx.x][1] = F[0].n_rai;
        halo[threadIdx.x][2] = F[0].q_lcl;
        halo[threadIdx.x][3] = F[0].n_lcl;
    }
    __syncthreads();
    if (!active || !owner) return;
    const int up = (threadIdx.x + 1 < nvalid) ? threadIdx.x + 1 : BS;
    const SedFlux<FT> above{halo[up][0], halo[up][1], halo[up][2], halo[up][3]};
    FT o[4][VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const SedFlux<FT> upf = (k + 1 < VEC) ? F[k + 1 < VEC ? k + 1 : 0] : above;
        const bool top = lev == io.n_lev - 1;
        // inflow through the upper face: the flux leaving the cell above (nothing enters through the model top)
        o[0][k] = A[k][0];
        o[1][k] = A[k][1];
        o[2][k] = top ? A[k][2] : M::fma(upf.q_rai, g[k], A[k][2]);
        o[3][k] = top ? A[k][3] : M::fma(upf.n_rai, g[k], A[k][3]);
        if constexpr (CLOUD) {
            o[0][k] = top ? A[k][0] : M::fma(upf.q_lcl, g[k], A[k][0]);
            o[1][k] = top ? A[k][1] : M::fma(upf.n_lcl, g[k], A[k][1]);
        }
        if (lev == 0 && io.precip) io.precip[col] = F[k].q_rai;             // surface precipitation flux of the column
        if (++lev == io.n_lev) { lev = 0; ++col; }
    }
    store_col<FT, VEC, true>(io.dq_lcl + first, v, o[0]);
    store_col<FT, VEC, true>(io.dn_lcl + first, v, o[1]);
    store_col<FT, VEC, true>(io.dq_rai + first, v, o[2]);
    store_col<FT, VEC, true>(io.dn_rai + first, v, o[3]);
