// snn_plasticity.inc -- the outer-product plasticity kernel of snn_ops.hip, included three times:
//   SNN_PLASTICITY_PV 0: k_plasticity<TJ>(StdpArgs) -- scalar learning rates and bounds; its text is what it was before the per-synapse
//                        instance existed, line for line, so that its code does not change;
//   SNN_PLASTICITY_PV 1: k_plasticity_pv<TJ>(StdpArgs, snn_synparams) -- every element reads its own rates and bounds through syn_at()
//                        and finishes through the bodies of snn_synparams.hpp.  Same 16 x TJ tiles: consecutive threads on consecutive
//                        columns, so W and an [S, N] constant are coalesced row-major streams, a [N] vector is re-read by the tile's
//                        rows from L1 / L2 and never becomes a full-matrix stream.  a.nu0 / a.nu1 hold, for a rate given as a tensor,
//                        1 or 0: whether any of its entries is non-zero (the reference's `nu[i].any()`); PostPre's rates multiply the
//                        staged [B, TJ] target factors and so vary by column only.
//   SNN_PLASTICITY_PV 2: k_plasticity_red<TJ, ACC>(StdpArgs, snn_synparams) -- the per-synapse text with the batch accumulator ACC in
//                        OuterSum's place (BatchReduce<R> of snn_order.hpp: reduction = torch.mean / amax / amin, snnhip.h f15).  Scalar
//                        rates and bounds reach it through syn_at()'s scalar side, so these reductions need no instance of their own of
//                        the scalar text.  SNN_PLASTICITY_ACC is OuterSum in the two sum instances: after preprocessing their token
//                        streams are what they were.  The assume_clamped skips stay valid: a reduction of zeros only is zero.
#if SNN_PLASTICITY_PV == 2
#define SNN_PLASTICITY_ACC ACC
template <int TJ, class ACC>
__global__ __launch_bounds__(256) void k_plasticity_red(StdpArgs a, snn_synparams q) {
#elif SNN_PLASTICITY_PV
#define SNN_PLASTICITY_ACC OuterSum
template <int TJ>
__global__ __launch_bounds__(256) void k_plasticity_pv(StdpArgs a, snn_synparams q) {
#else
#define SNN_PLASTICITY_ACC OuterSum
template <int TJ>
__global__ __launch_bounds__(256) void k_plasticity(StdpArgs a) {
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int B = a.B, Nin = a.Nin, N = a.N;
    const int MW = (B + 31) / 32;                       // mask words per row / column
    float *xt = (float *)smem;                          // [B][TJ]  target-side float factor
    float *xs = xt + (size_t)B * TJ;                    // [B][kTI] source-side float factor
    uint32_t *mT = (uint32_t *)(xs + (size_t)B * kTI);  // [TJ][MW] target spike masks
    uint32_t *mS = mT + (size_t)TJ * MW;                // [kTI][MW]
    uint8_t *vT = (uint8_t *)(mS + (size_t)kTI * MW);   // [B][TJ] target spike values
    uint8_t *vS = vT + (size_t)B * TJ;                  // [B][kTI]
    __shared__ int any_flag;

    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * TJ, i0 = blockIdx.y * kTI;
    if (tid == 0) any_flag = 0;
    __syncthreads();
    int local_any = 0;
    for (int k = tid; k < B * TJ; k += 256) {
        const int b = k / TJ, jj = k - b * TJ, j = j0 + jj;
        float f = 0.f; uint8_t sv = 0;
        if (j < N) {
            sv = a.s_tgt[(size_t)b * N + j];
            f = a.x_tgt[(size_t)b * N + j];
#if SNN_PLASTICITY_PV
            if (a.mode == 0) f = f * syn_at(q.nu0, 0, q.nu0_cs, a.nu0, 0, j);      // target_x * nu[0], the column's own rate
#else
            if (a.mode == 0) f = f * a.nu0;             // target_x * nu[0]  (MCC_learning.py:235)
#endif
        }
        xt[k] = f; vT[k] = sv; local_any |= sv;
    }
    for (int k = tid; k < B * kTI; k += 256) {
        const int b = k / kTI, ii = k - b * kTI, i = i0 + ii;
        float f = 0.f; uint8_t sv = 0;
        if (i < Nin) { sv = a.s_src[(size_t)b * Nin + i]; f = a.x_src[(size_t)b * Nin + i]; }
        xs[k] = f; vS[k] = sv; local_any |= sv;
    }
    if (local_any) any_flag = 1;
    __syncthreads();
    if (a.assume_clamped && !any_flag) return;          // nothing in this tile can change
    for (int k = tid; k < (TJ + kTI) * MW; k += 256) {
        const bool tgt = k < TJ * MW;
        const int kk = tgt ? k : k - TJ * MW;
        const int col = kk / MW, w = kk - col * MW;
        uint32_t m = 0;
        for (int bit = 0; bit < 32; ++bit) {
            const int b = w * 32 + bit;
            if (b < B && (tgt ? vT[(size_t)b * TJ + col] : vS[(size_t)b * kTI + col])) m |= 1u << bit;
        }
        (tgt ? mT : mS)[kk] = m;
    }
    __syncthreads();

    const long E = (long)Nin * N, Emain = (E / 32) * 32;
    constexpr int RG = 256 / TJ;                        // row groups handled concurrently
    const int jj = tid % TJ, rg = tid / TJ, j = j0 + jj;
    if (j >= N) return;
    for (int ii = rg; ii < kTI; ii += RG) {
        const int i = i0 + ii;
        if (i >= Nin) break;
        uint32_t anyS = 0, anyT = 0;
        for (int w = 0; w < MW; ++w) { anyS |= mS[ii * MW + w]; anyT |= mT[jj * MW + w]; }
        if (a.assume_clamped && !anyS && !anyT) continue;
        const long e = (long)i * N + j;
        const bool tail = e >= Emain;
        float w_ = a.W[e];
#if SNN_PLASTICITY_PV
        const SynElem c = syn_elem(q, a.nu0, a.nu1, a.has_min, a.wmin, a.has_max, a.wmax, i, j);
#endif
        if (a.mode == 0) {
            if (a.nu0 != 0.f) {                         // pre: sum_b s_src[b,i] * (x_tgt[b,j]*nu0)
                SNN_PLASTICITY_ACC acc; acc.init(tail);
                for (int w = 0; w < MW; ++w) {
                    uint32_t m = mS[ii * MW + w];
                    while (m) {
                        const int b = w * 32 + __ffs(m) - 1; m &= m - 1;
                        acc.add(b, (float)vS[(size_t)b * kTI + ii] * xt[(size_t)b * TJ + jj], B);
                    }
                }
                float u = acc.finish(B);
#if SNN_PLASTICITY_PV
                w_ = syn_postpre(w_, true, u, false, 0.f, a.use_dt, a.dt);
#else
                if (a.use_dt) u = u * a.dt;
                w_ = w_ - u;
#endif
            }
            if (a.nu1 != 0.f) {                         // post: sum_b x_src[b,i] * (s_tgt[b,j]*nu1)
                SNN_PLASTICITY_ACC acc; acc.init(tail);
                for (int w = 0; w < MW; ++w) {
                    uint32_t m = mT[jj * MW + w];
                    while (m) {
                        const int b = w * 32 + __ffs(m) - 1; m &= m - 1;
#if SNN_PLASTICITY_PV
                        const float st = (float)vT[(size_t)b * TJ + jj] * c.nu1;
#else
                        const float st = (float)vT[(size_t)b * TJ + jj] * a.nu1;
#endif
                        acc.add(b, xs[(size_t)b * kTI + ii] * st, B);
                    }
                }
                float u = acc.finish(B);
#if SNN_PLASTICITY_PV
                w_ = syn_postpre(w_, false, 0.f, true, u, a.use_dt, a.dt);
#else
                if (a.use_dt) u = u * a.dt;
                w_ = w_ + u;
#endif
            }
        } else if (a.mode == 2 || a.mode == 3) {
            float u1 = 0.f, u2 = 0.f;
            {   // U1 = sum_b s_src[b,i] * x_tgt[b,j]
                SNN_PLASTICITY_ACC acc; acc.init(tail);
                for (int w = 0; w < MW; ++w) {
                    uint32_t m = mS[ii * MW + w];
                    while (m) { const int b = w * 32 + __ffs(m) - 1; m &= m - 1; acc.add(b, (float)vS[(size_t)b * kTI + ii] * xt[(size_t)b * TJ + jj], B); }
                }
                u1 = acc.finish(B);
            }
            {   // U2 = sum_b x_src[b,i] * s_tgt[b,j]
                SNN_PLASTICITY_ACC acc; acc.init(tail);
                for (int w = 0; w < MW; ++w) {
                    uint32_t m = mT[jj * MW + w];
                    while (m) { const int b = w * 32 + __ffs(m) - 1; m &= m - 1; acc.add(b, xs[(size_t)b * kTI + ii] * (float)vT[(size_t)b * TJ + jj], B); }
                }
                u2 = acc.finish(B);
            }
#if SNN_PLASTICITY_PV
            w_ = a.mode == 2 ? syn_hebbian(w_, u1, u2, c.nu0, c.nu1)
                             : syn_wdpostpre(w_, a.nu0 != 0.f, u1, a.nu1 != 0.f, u2, c.nu0, c.nu1, c.lo, c.hi);
#else
            if (a.mode == 2) {                          // w += nu0 * U1; w += nu1 * U2
                w_ = w_ + a.nu0 * u1;
                w_ = w_ + a.nu1 * u2;
            } else {                                    // update = 0 - (nu0 U1)(w - wmin) + (nu1 U2)(wmax - w); w += update
                float upd = 0.f; bool have = false;
                if (a.nu0 != 0.f) { upd = 0.0f - (a.nu0 * u1) * (w_ - a.wmin); have = true; }
                if (a.nu1 != 0.f) { const float y = (a.nu1 * u2) * (a.wmax - w_); upd = have ? upd + y : y; have = true; }
                if (have) w_ = w_ + upd;
            }
#endif
        } else {                                        // MSTDP: sum_b reward * elig[b][i,j]
            SNN_PLASTICITY_ACC acc; acc.init(tail);
            for (int w = 0; w < MW; ++w) {
                uint32_t m = mS[ii * MW + w] | mT[jj * MW + w];
                while (m) {
                    const int b = w * 32 + __ffs(m) - 1; m &= m - 1;
                    const float e1 = xs[(size_t)b * kTI + ii] * (float)vT[(size_t)b * TJ + jj];   // p_plus (x) s_tgt
                    const float e2 = (float)vS[(size_t)b * kTI + ii] * xt[(size_t)b * TJ + jj];   // s_src (x) p_minus
                    const float el = e1 + e2;
                    const float r = a.reward_vec ? a.reward_vec[b] : a.reward;
                    acc.add(b, r * el, B);
                }
            }
            const float u = acc.finish(B);
#if SNN_PLASTICITY_PV
            w_ = syn_mstdp(w_, u, c.nu0);
#else
            w_ = w_ + a.nu0 * u;                        // learning.py:1561
#endif
        }
#if SNN_PLASTICITY_PV
        a.W[e] = syn_finish(w_, a.decay, c.lo, c.hi);
#else
        w_ = w_ * a.decay;
        if (a.has_min && w_ < a.wmin) w_ = a.wmin;
        if (a.has_max && w_ > a.wmax) w_ = a.wmax;
        a.W[e] = w_;
#endif
    }
}
#undef SNN_PLASTICITY_ACC
