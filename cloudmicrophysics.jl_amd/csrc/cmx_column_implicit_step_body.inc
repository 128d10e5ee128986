// cmx_column_implicit_step_body.inc — the body of implicit_sedimentation_step_kernel (cmx_column_implicit_step.hip) and of its ensemble form
// (cmx_column_implicit_step_ensemble.hip), shared as TEXT: a __device__ template around a kernel body moved registers in a tenth of the instantiations
// when the §(29) entries were built (HISTORY.md), the same lines included twice moved none.  The including kernel has the template parameters
// S, FX, FT, K, BS and defines
//   CMX_ISTEP_TEND_CONSTS        the tendency constants, as implicit_average_substeps takes them
//   CMX_ISTEP_FLUX_CONSTS        the flux side's constants (FX::fluxes reads them phase by phase: front_consts<FT, true>, consts_after)
//   CMX_ISTEP_AVG_ARGS           the ImplicitAverageArgs of the substeps: h, 1/h, 1/Δt, nsub, the step flags, Lv, Ls
//   CMX_ISTEP_IO0                the IO struct as the kernel argument holds it, for what is needed BEFORE the substeps (the workgroup's range of columns)
//   CMX_ISTEP_ARGS_AFTER(dep)    the kernel argument's .a (output columns) and .io, read through the kernel-argument pointer AFTER `dep` is known
//   CMX_ISTEP_IN_INDEX(i)        the index into the input columns of flat point i of this workgroup's column set
//   CMX_ISTEP_COL_ORIGIN(io)     the first column of this workgroup's column set in the output columns and the surface fluxes
//   CMX_ISTEP_NT_IN              whether the input loads carry the non-temporal hint (a compile-time `true`, or wave-uniform)
    using M = Math<FT>;
    constexpr int N = S::NOUT, S0 = 1 + S::SPECIES0;
    static_assert(N == 4 && S0 + N == S::NWRT + 1, "implicit_sedimentation_step_kernel: four species, the last four inputs of the point");
    __shared__ __align__(16) FT As[BS][N], Bs[BS][N], Gs[BS][N];      // A, B and G of every point of the chunk
    __shared__ FT carry[2][N];                                        // G of the point above the chunk, per species; the slots alternate from chunk to chunk
    const auto &a = CMX_ISTEP_AVG_ARGS;
    // the workgroup's range of whole columns: P points from flat index `base`
    const int64_t col0 = (int64_t)blockIdx.x * CMX_ISTEP_IO0.cols_per_wg;
    const int64_t left = CMX_ISTEP_IO0.n_col - col0;
    const uint32_t P = (uint32_t)(left < CMX_ISTEP_IO0.cols_per_wg ? left : (int64_t)CMX_ISTEP_IO0.cols_per_wg) * (uint32_t)CMX_ISTEP_IO0.n_lev;
    const int64_t base = col0 * CMX_ISTEP_IO0.n_lev;
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS (every lane of the workgroup reaches the barrier inside); no-op for Float32
    uint32_t par = 0;
#pragma unroll 1
    for (uint32_t cs = (P - 1) / BS * BS;; cs -= BS) {      // chunks [cs, cs + BS) ∩ [0, P) of the range, the highest first
        const uint32_t rel = cs + threadIdx.x;
        const bool active = rel < P;
        const int64_t i = base + rel;
        FT hq[N], rr[N], g = FT(0);
        uint32_t lev = 0, relcol = 0;
        bool top = false;
        if (active) {
            FT x[S::NWRT + 1], s0[N], avg[N], F[N], w[N];
            if (CMX_ISTEP_NT_IN) {
#pragma unroll
                for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + CMX_ISTEP_IN_INDEX(i));
            } else {
#pragma unroll
                for (int j = 0; j < S::NWRT + 1; ++j) x[j] = a.in[j][CMX_ISTEP_IN_INDEX(i)];
            }
#pragma unroll
            for (int q = 0; q < N; ++q) s0[q] = x[S0 + q];
            implicit_average_substeps<S, FT, K>(CMX_ISTEP_TEND_CONSTS, a, x, avg);
            // ---- fluxes and fall speeds of the INITIAL state
            {
                const auto &kq = CMX_ISTEP_ARGS_AFTER(avg[N - 1]);
                const int32_t opt[2] = {kq.io.opt[0], kq.io.opt[1]};
                FX::fluxes(CMX_ISTEP_FLUX_CONSTS, avg[N - 1], opt, x[0], s0, F, w);
            }
            const auto &kp = CMX_ISTEP_ARGS_AFTER(F[N - 1]);
            const auto &io = kp.io;
            const FastDivU32 dv{io.lev_div.magic, io.lev_div.sh1, io.lev_div.sh2, io.lev_div.d};
            relcol = fastdiv(rel, dv);
            lev = rel - relcol * (uint32_t)io.n_lev;
            top = lev == (uint32_t)io.n_lev - 1;          // nothing enters through the model top
            const FT idz = io.inv_dz[lev];
            const FT rp = max0(x[0]);
            g = idz * FX::inv_rho(x[0]);                  // 1/(ρ_k Δz_k)
            const int32_t opt[2] = {io.opt[0], io.opt[1]};
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const FT tau = io.dt * w[q];
                const FT c = tau * idz, beta = tau * rp;
                const FT r = FT(1) / (FT(1) + c);         // a true division: exactly 1 at c = 0
                As[threadIdx.x][q] = c * r;
                Bs[threadIdx.x][q] = M::fma(beta, avg[q], F[q]) * r;
                rr[q] = r;
                hq[q] = FX::falls(q, opt) ? M::fma(-F[q], g, avg[q]) : avg[q];
            }
        }
        __syncthreads();
        {   // ---- the chains of the chunk: lane → (segment = the part of one column inside the chunk, species)
            const auto &io = CMX_ISTEP_ARGS_AFTER(g).io;
            const uint32_t n_lev = (uint32_t)io.n_lev;
            const uint32_t ce = cs + BS < P ? cs + BS : P;
            const FastDivU32 dv{io.lev_div.magic, io.lev_div.sh1, io.lev_div.sh2, io.lev_div.d};
            const uint32_t colA = fastdiv(cs, dv), nseg = fastdiv(ce - 1, dv) - colA + 1;
            for (uint32_t sl = threadIdx.x; sl < nseg * N; sl += BS) {
                const uint32_t q = sl % N, col = colA + sl / N;
                const uint32_t cb = col * n_lev, ct = cb + n_lev;       // the column: [cb, ct) of the range
                const uint32_t lo = cb > cs ? cb : cs, hi = ct < ce ? ct : ce;
                const bool from_top = hi == ct;
                uint32_t p = hi - 1 - cs;
                const FT Gup = carry[par][q];
                FT G = from_top ? Bs[p][q] : M::fma(As[p][q], Gup, Bs[p][q]);      // a select: nothing crosses a column top
                Gs[p][q] = G;
#pragma unroll 4
                for (uint32_t m = hi - lo - 1; m > 0; --m) {
                    --p;
                    G = M::fma(As[p][q], G, Bs[p][q]);
                    Gs[p][q] = G;
                }
                if (lo > cb) carry[par ^ 1][q] = G;       // the column goes on in the next chunk
            }
        }
        __syncthreads();
        if (active) {
            const auto &kp = CMX_ISTEP_ARGS_AFTER(g);
            const auto &io = kp.io;
            const int32_t opt[2] = {io.opt[0], io.opt[1]};
            const int64_t origin = CMX_ISTEP_COL_ORIGIN(io);
#pragma unroll
            for (int q = 0; q < N; ++q) {
                FT up = FT(0);
                if (!top) up = threadIdx.x == BS - 1 ? carry[par][q] : Gs[threadIdx.x + 1 < BS ? threadIdx.x + 1 : 0][q];
                const FT o = M::fma(up, g, hq[q]) * rr[q];
                kp.a.avg[q][origin * io.n_lev + i] = FX::falls(q, opt) ? o : hq[q];
            }
            if (lev == 0) {                               // the flux that leaves the column during the step
                const int64_t col = origin + col0 + relcol;
                if constexpr (FX::precip(0) >= 0)
                    if (io.precip[0]) io.precip[0][col] = Gs[threadIdx.x][FX::precip(0)];
                if constexpr (FX::precip(1) >= 0)
                    if (io.precip[1]) io.precip[1][col] = Gs[threadIdx.x][FX::precip(1)];
            }
        }
        par ^= 1;
        if (cs == 0) break;
    }
