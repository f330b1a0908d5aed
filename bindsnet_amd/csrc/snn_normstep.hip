// snn_normstep.hip -- snn_prop_cascade_norm_f32 / snn_prop_cascade_norm_pv_f32: Weight(norm_frequency="time step"), the propagation of
// a MulticompartmentConnection with one Weight and the normalisation of that Weight in ONE launch (topology_features.py:633-645).
//
// grid ceil(N / kPnCols), 256 threads.  A workgroup owns kPnCols columns of W with all Nin rows: the tile is read from memory once
// into LDS, its column sums are formed (ATen's sum(dim=0) order), every sample's currents are summed from the OLD weights (k_prop's
// event-driven walk, ATen's sum(dim=1) order), and the tile is written back scaled -- each weight is loaded once and stored once,
// where the two calls load it three times (k_prop's rows, k_colsum, k_scale_cols).  The columns are independent of each other, so
// no workgroup waits for another.  All arithmetic is the text of snn_normstep.hpp.
// A tile that does not fit the LDS (Nin above ~1100 rows) takes the two calls.
// Measured at 784 x 400, B = 32 (profiles/NOTES_norm_step.md) the launch is SLOWER than the three it replaces -- 25 workgroups walk
// 32 samples' lists each while k_prop spreads them over 64 -- so snn_net_run calls it only for snn_conn_desc.norm_step == 2 and
// Network.run asks for the two calls; the entry points stay as operators (ops.prop_cascade_norm).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_normstep.hpp"

using namespace snn;

template <bool NV>
__global__ __launch_bounds__(kPnThreads) void k_prop_norm(float *W, const uint8_t *__restrict__ s, float *__restrict__ out, int B, int Nin,
                                                          int N, int accumulate, float norm, const float *__restrict__ norm_vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nbs = pn_blocks_per_col(Nin) + 1;
    float *tile = (float *)smem;                               // [Nin][kPnCols]
    float *bs = tile + (size_t)Nin * kPnCols;                  // [kPnCols][nbs]
    float *seq = bs + (size_t)nbs * kPnCols;                   // [kPnCols][4]
    float *scale = seq + 4 * kPnCols;                          // [kPnCols]
    uint32_t *list = (uint32_t *)(scale + kPnCols);            // [kPnSamples][Nin]
    int *cnt = (int *)(list + (size_t)kPnSamples * Nin);       // [kPnSamples]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * kPnCols;
    const int total = Nin * kPnCols;
    for (int idx = tid; idx < total; idx += kPnThreads) {      // a column past N repeats the last one; it is never stored
        const int i = idx / kPnCols, j = j0 + idx % kPnCols;
        tile[idx] = W[(size_t)i * N + (j < N ? j : N - 1)];
    }
    __syncthreads();
    for (int it = tid; it < (Nin >> 4) * kPnCols; it += kPnThreads) {
        const int c = it % kPnCols, r = it / kPnCols;
        const bool tail = outer_tail(j0 + c, N);
        if (r < pn_block_items(tail, Nin)) bs[c * nbs + r] = pn_block_sum(tile, c, tail, r);
    }
    __syncthreads();
    if (tid < 4 * kPnCols) {
        const int c = tid % kPnCols, q = tid / kPnCols;
        const bool tail = outer_tail(j0 + c, N);
        if (tail || q == 0) seq[c * 4 + q] = pn_seq_fold(bs + c * nbs, tile, c, tail, q, Nin);
    }
    __syncthreads();
    if (tid < kPnCols) {
        const int j = j0 + tid;
        const float cs = pn_colsum(seq + tid * 4, tile, tid, outer_tail(j, N), Nin);
        scale[tid] = NV ? pn_scale_pv(cs, norm_vec[j < N ? j : N - 1]) : pn_scale(cs, norm);
    }
    // the currents, kPnSamples samples a pass: wave w compacts the spikes of samples 4w .. 4w + 3 into ascending lists, then thread
    // (sample, column) walks its sample's list
    const uint64_t lt = (1ull << lane) - 1ull;
    const int bl = tid / kPnCols, c = tid % kPnCols, j = j0 + c;
    const bool tail = outer_tail(j, N);
    for (int b0 = 0; b0 < B; b0 += kPnSamples) {
        for (int u = 0; u < 4; ++u) {
            const int l = wave * 4 + u, b = b0 + l;
            uint32_t *mine = list + (size_t)l * Nin;
            int n = 0;
            if (b < B) {
                const uint8_t *srow = s + (size_t)b * Nin;
                for (int base = 0; base < Nin; base += 64) {
                    const int i = base + lane;
                    const uint32_t sv = i < Nin ? srow[i] : 0u;
                    const uint64_t m = __ballot(sv != 0);
                    if (sv) mine[n + __popcll(m & lt)] = ((uint32_t)i << 8) | sv;
                    n += __popcll(m);
                }
            }
            if (lane == 0) cnt[l] = n;
        }
        __syncthreads();
        const int b = b0 + bl;
        if (b < B && j < N) {
            const float r = pn_current(tile, c, list + (size_t)bl * Nin, cnt[bl], Nin, tail);
            const size_t o = (size_t)b * N + j;
            out[o] = (accumulate ? out[o] : 0.0f) + r;
        }
        __syncthreads();
    }
    for (int idx = tid; idx < total; idx += kPnThreads) {
        const int i = idx / kPnCols, cc = idx % kPnCols;
        if (j0 + cc < N) W[(size_t)i * N + j0 + cc] = tile[idx] * scale[cc];
    }
}

// N == 1: one workgroup; every sample's current first (k_prop_col1's inner reduction), then the column's sum, then the scaling
template <bool NV>
__global__ __launch_bounds__(256) void k_prop_norm_col1(float *W, const uint8_t *__restrict__ s, float *__restrict__ out, int B, int Nin,
                                                        int accumulate, float norm, const float *__restrict__ norm_vec) {
    __shared__ float sc;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float r = pn_col1_current(W, s + (size_t)b * Nin, Nin);
        out[b] = (accumulate ? out[b] : 0.0f) + r;
    }
    if (threadIdx.x == 0) {
        const float cs = pn_col1_sum(W, Nin);
        sc = NV ? pn_scale_pv(cs, norm_vec[0]) : pn_scale(cs, norm);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < Nin; i += 256) W[i] = W[i] * sc;
}

static constexpr size_t kPnMaxLds = 150 * 1024;

template <bool NV>
static int prop_norm(float *W, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate, float norm, const float *norm_vec,
                     float *colsum_ws, hipStream_t st) {
    if (!W || !s || !out || !colsum_ws || (NV && !norm_vec) || B <= 0 || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (Nin > kMaxTerms || B > 65535) return SNN_ERR_UNSUPPORTED;
    if (N == 1) {
        hipLaunchKernelGGL(k_prop_norm_col1<NV>, dim3(1), dim3(256), 0, st, W, s, out, B, Nin, accumulate, norm, norm_vec);
        return snn_check_launch();
    }
    const size_t lds = pn_lds_bytes(Nin);
    if (lds > kPnMaxLds) {                                 // the tile does not fit: the two calls (the same bits by contract)
        const int rc = snn_prop_cascade_f32(W, s, out, B, Nin, N, accumulate, (snn_stream_t)st);
        if (rc) return rc;
        return NV ? snn_normalize_pv(W, Nin, N, norm_vec, 0, colsum_ws, (snn_stream_t)st)
                  : snn_normalize(W, Nin, N, norm, 0, colsum_ws, (snn_stream_t)st);
    }
    static int state = 0;                                  // (process-wide: the attribute belongs to the function)
    if (!state) state = snn_check(hipFuncSetAttribute((const void *)k_prop_norm<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPnMaxLds)) ||
                        snn_check(hipFuncSetAttribute((const void *)k_prop_norm<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPnMaxLds)) ? -1 : 1;
    if (state < 0) return SNN_ERR_LAUNCH;
    hipLaunchKernelGGL(k_prop_norm<NV>, dim3((N + kPnCols - 1) / kPnCols), dim3(kPnThreads), lds, st, W, s, out, B, Nin, N, accumulate, norm,
                       norm_vec);
    return snn_check_launch();
}

extern "C" int snn_prop_cascade_norm_f32(float *W, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate, float norm,
                                         float *colsum_ws, snn_stream_t stream) {
    return prop_norm<false>(W, s, out, B, Nin, N, accumulate, norm, nullptr, colsum_ws, (hipStream_t)stream);
}

extern "C" int snn_prop_cascade_norm_pv_f32(float *W, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate,
                                            const float *norm_vec, float *colsum_ws, snn_stream_t stream) {
    return prop_norm<true>(W, s, out, B, Nin, N, accumulate, 0.f, norm_vec, colsum_ws, (hipStream_t)stream);
}
