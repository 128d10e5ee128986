// cmx_mp1m_tend_body.inc — the body of mp1m_tendencies_kernel (cmx_mp1m_kernels.hip has the story), as text: the ensemble kernel
// (cmx_mp1m_ensemble.hip) includes the same lines, so both forms are the same operations on the same operands.  The including kernel provides
//   FT, VEC, FLAGS                    the template parameters of mp1m_tendencies_kernel
//   in, out, nvec                     Mp1mIn<FT>, Mp1mOut<FT> and the number of vectors that blockIdx.x tiles
//   CMX_MP1M_TEND_CONSTS(ALSO)        the constants: an expression the point function takes as its first argument
//   CMX_MP1M_TEND_NT_IN               whether the input loads carry the non-temporal hint
    const int64_t i = (int64_t)blockIdx.x * kBlock1m<FT> + threadIdx.x;
    FT rho[VEC], T[VEC], q_tot[VEC], q_lcl[VEC], q_icl[VEC], q_rai[VEC], q_sno[VEC];
    if (i < nvec) {
        load_col<FT, VEC, CMX_MP1M_TEND_NT_IN>(in.rho, i, rho); load_col<FT, VEC, CMX_MP1M_TEND_NT_IN>(in.T, i, T); load_col<FT, VEC, CMX_MP1M_TEND_NT_IN>(in.q_tot, i, q_tot);
        load_col<FT, VEC, CMX_MP1M_TEND_NT_IN>(in.q_lcl, i, q_lcl); load_col<FT, VEC, CMX_MP1M_TEND_NT_IN>(in.q_icl, i, q_icl); load_col<FT, VEC, CMX_MP1M_TEND_NT_IN>(in.q_rai, i, q_rai);
        load_col<FT, VEC, CMX_MP1M_TEND_NT_IN>(in.q_sno, i, q_sno);
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS while the loads fly (every lane of the workgroup reaches the barrier inside); no-op for Float32
    if (i >= nvec) return;
    FT dl[VEC], di[VEC], dr[VEC], ds[VEC];
    if constexpr (sizeof(FT) == 4 && VEC == 4) {
        // Float32, four points per lane: two PAIRS of points in packed arithmetic (cmx_math.hpp f32x2); the constants are read phase by phase through the
        // kernel-argument pointer (a packed instruction takes no literal: the point function's literals occupy SGPRs next to the constants).
        // Rounds 1–4 evaluated one point at a time here; round 3 parked the additive constants of every `a·x + b` in VGPRs once per lane for
        // them (an instruction reads one SGPR: 12 of a point's 266 instructions were v_mov_b32 of b; 70 → 76 VGPRs, 0.782–0.793 → 0.778–0.779 ms
        // per 1e8 points) — the packed form took over every instantiation that did.
#pragma unroll
        for (int k = 0; k < VEC; k += 2) {
            f32x2 l, ic, r, sn;
            mp1m_tendencies_point<f32x2, FLAGS>(CMX_MP1M_TEND_CONSTS(true), f32x2{rho[k], rho[k + 1]}, f32x2{T[k], T[k + 1]}, f32x2{q_tot[k], q_tot[k + 1]},
                                                f32x2{q_lcl[k], q_lcl[k + 1]}, f32x2{q_icl[k], q_icl[k + 1]}, f32x2{q_rai[k], q_rai[k + 1]},
                                                f32x2{q_sno[k], q_sno[k + 1]}, l, ic, r, sn);
            dl[k] = l.x; dl[k + 1] = l.y; di[k] = ic.x; di[k + 1] = ic.y; dr[k] = r.x; dr[k + 1] = r.y; ds[k] = sn.x; ds[k + 1] = sn.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            mp1m_tendencies_point<FT, FLAGS>(CMX_MP1M_TEND_CONSTS(FLAGS == kRuntimeFlags), rho[k], T[k], q_tot[k], q_lcl[k], q_icl[k], q_rai[k], q_sno[k], dl[k],
                                             di[k], dr[k], ds[k]);
    }
    store_col<FT, VEC>(out.dq_lcl, i, dl); store_col<FT, VEC>(out.dq_icl, i, di);
    store_col<FT, VEC>(out.dq_rai, i, dr); store_col<FT, VEC>(out.dq_sno, i, ds);
