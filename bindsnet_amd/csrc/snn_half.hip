// snn_half.hip -- float16 / bfloat16 Weight features on gfx950: the three kernels of a MulticompartmentConnection whose single
// Weight.value is 2 bytes wide (snn_half.hpp states the arithmetic).  Everything is float32 arithmetic behind explicit
// conversions; the weights are read and written with 2-byte accesses, lane <-> column, so a wave touches 128 contiguous bytes
// of a row whatever the row's alignment (rows of an odd N start on 2-byte boundaries: no wider access is used).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_half.hpp"

using namespace snn;

// =============================================================================================
// Propagation: k_prop of snn_ops.hip over 2-byte weights.  grid (ceil(N/256), B), thread <-> target column, block <-> sample;
// per 1024-source chunk every wave compacts its sources into an ascending list, the threads walk the lists.
// =============================================================================================
template <int DT>
__global__ __launch_bounds__(256) void k_prop_h16(const uint16_t *__restrict__ W, const uint8_t *__restrict__ s, float *__restrict__ out,
                                                  int B, int Nin, int N, int accumulate) {
    __shared__ uint32_t list[4][256];
    __shared__ int cnt[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y, j = blockIdx.x * 256 + tid;
    const bool valid = j < N;
    const int jc = valid ? j : N - 1;
    const uint8_t *srow = s + (size_t)b * Nin;
    OuterSum acc;
    acc.init(outer_tail(j, N));
    const uint64_t lt = (1ull << lane) - 1ull;

    for (int base = 0; base < Nin; base += 1024) {
        int n_w = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = base + wave * 256 + p * 64 + lane;
            const uint32_t sv = (i < Nin) ? srow[i] : 0u;
            const uint64_t m = __ballot(sv != 0);
            if (sv) list[wave][n_w + __popcll(m & lt)] = ((uint32_t)i << 8) | sv;
            n_w += __popcll(m);
        }
        if (lane == 0) cnt[wave] = n_w;
        __syncthreads();
        for (int w = 0; w < 4; ++w) {
            const int n = cnt[w];
            for (int k = 0; k < n; k += 4) {
                uint32_t e[4]; uint16_t wv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    e[u] = list[w][(k + u < n) ? k + u : k];
                    wv[u] = W[(size_t)(e[u] >> 8) * N + jc];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + u < n) acc.add((int)(e[u] >> 8), half_widen<DT>(wv[u]) * (float)(e[u] & 255u), Nin);
            }
        }
        __syncthreads();
    }
    if (valid) {
        const size_t o = (size_t)b * N + j;
        out[o] = half_prop_finish<DT>(acc.finish(Nin), accumulate ? out[o] : 0.0f, accumulate);
    }
}

extern "C" int snn_prop_cascade_h16(const void *W, int w_dtype, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate,
                                    snn_stream_t stream) {
    if (!W || !s || !out || B <= 0 || Nin <= 0 || N <= 0 || (w_dtype != kWF16 && w_dtype != kWBF16)) return SNN_ERR_INVALID;
    if (Nin > kMaxTerms || B > 65535) return SNN_ERR_UNSUPPORTED;
    const dim3 grid((N + 255) / 256, B);
    if (w_dtype == kWF16)
        hipLaunchKernelGGL(k_prop_h16<kWF16>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t *)W, s, out, B, Nin, N, accumulate);
    else
        hipLaunchKernelGGL(k_prop_h16<kWBF16>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t *)W, s, out, B, Nin, N, accumulate);
    return snn_check_launch();
}

// =============================================================================================
// PostPre.  Workgroup = 256 consecutive columns x a strip of kPpRows rows.  The spike bits of the strip's source rows and of the
// workgroup's columns go to LDS once (one bit per sample); every thread then owns one column and walks the strip's rows, so the
// weights of a row are read and written as one run of 2-byte elements per wave.
// =============================================================================================
constexpr int kPpRows = 16;

template <int DT, int R = kReduceSum>
__global__ __launch_bounds__(256) void k_postpre_h16(uint16_t *__restrict__ W, const HalfPostPre a) {
    __shared__ uint32_t mS[kPpRows][kHalfMaskWords];
    __shared__ uint32_t mT[kHalfMaskWords][256];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * kPpRows, j = blockIdx.x * 256 + tid;
    const int MW = (a.B + 31) / 32;
    for (int k = tid; k < kPpRows * kHalfMaskWords; k += 256) mS[k / kHalfMaskWords][k % kHalfMaskWords] = 0u;
    for (int w = 0; w < MW; ++w) {                     // the column's target spikes: one coalesced byte row per sample
        uint32_t m = 0;
        for (int bb = 0; bb < 32; ++bb) {
            const int b = w * 32 + bb;
            if (b < a.B && j < a.N && a.s_tgt[(size_t)b * a.N + j]) m |= 1u << bb;
        }
        mT[w][tid] = m;
    }
    __syncthreads();
    for (int k = tid; k < kPpRows * a.B; k += 256) {   // the strip's source spikes
        const int r = k % kPpRows, b = k / kPpRows, i = i0 + r;
        if (i < a.Nin && a.s_src[(size_t)b * a.Nin + i]) atomicOr(&mS[r][b >> 5], 1u << (b & 31));
    }
    __syncthreads();
    if (j >= a.N) return;
    for (int r = 0; r < kPpRows; ++r) {
        const int i = i0 + r;
        if (i >= a.Nin) break;
        const size_t e = (size_t)i * a.N + j;
        W[e] = half_postpre_elem<DT, R>(W[e], a, i, j, &mS[r][0], 1, &mT[0][tid], 256);
    }
}

template <int DT>
static void launch_postpre_h16(int reduce, dim3 grid, hipStream_t st, uint16_t *W, const HalfPostPre &a) {
    auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, W, a); };
    if (reduce == SNN_REDUCE_MEAN) launch(k_postpre_h16<DT, kReduceMean>);
    else if (reduce == SNN_REDUCE_AMAX) launch(k_postpre_h16<DT, kReduceAmax>);
    else if (reduce == SNN_REDUCE_AMIN) launch(k_postpre_h16<DT, kReduceAmin>);
    else launch(k_postpre_h16<DT>);
}

extern "C" int snn_stdp_postpre_h16_red(void *W, int w_dtype, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                                        const float *x_tgt, int B, int Nin, int N, float nu0, float nu1, int use_dt, float dt, float decay,
                                        int has_min, float wmin, int has_max, float wmax, int reduce, snn_stream_t stream) {
    if (reduce < SNN_REDUCE_SUM || reduce > SNN_REDUCE_AMIN) return SNN_ERR_INVALID;
    if (!W || !s_src || !x_src || !s_tgt || !x_tgt || B <= 0 || Nin <= 0 || N <= 0 || (w_dtype != kWF16 && w_dtype != kWBF16)) return SNN_ERR_INVALID;
    if (B > kHalfMaxB || (Nin + kPpRows - 1) / kPpRows > 65535) return SNN_ERR_UNSUPPORTED;
    const HalfPostPre a{s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, use_dt, dt, decay, has_min, wmin, has_max, wmax};
    const dim3 grid((N + 255) / 256, (Nin + kPpRows - 1) / kPpRows);
    if (w_dtype == kWF16) launch_postpre_h16<kWF16>(reduce, grid, (hipStream_t)stream, (uint16_t *)W, a);
    else launch_postpre_h16<kWBF16>(reduce, grid, (hipStream_t)stream, (uint16_t *)W, a);
    return snn_check_launch();
}

extern "C" int snn_stdp_postpre_h16(void *W, int w_dtype, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                                    const float *x_tgt, int B, int Nin, int N, float nu0, float nu1, int use_dt, float dt, float decay,
                                    int has_min, float wmin, int has_max, float wmax, snn_stream_t stream) {
    return snn_stdp_postpre_h16_red(W, w_dtype, s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, use_dt, dt, decay, has_min, wmin, has_max, wmax,
                                    SNN_REDUCE_SUM, stream);
}

// =============================================================================================
// Normalise: one thread per column for the factor (64-thread workgroups, so the columns spread over the CUs), then one pass
// over the elements.  The factor travels as its float32 widening in the caller's column workspace.
// =============================================================================================
template <int DT>
__global__ __launch_bounds__(64) void k_norm_factor_h16(const uint16_t *__restrict__ W, int Nin, int N, float norm, float *__restrict__ factor) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j < N) factor[j] = half_norm_factor<DT>(W, Nin, N, j, norm);
}

template <int DT>
__global__ __launch_bounds__(256) void k_norm_scale_h16(uint16_t *__restrict__ W, long E, int N, const float *__restrict__ factor) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long)gridDim.x * 256) W[e] = half_norm_scale<DT>(W[e], factor[e % N]);
}

extern "C" int snn_normalize_h16(void *W, int w_dtype, int Nin, int N, float norm, float *colsum_ws, snn_stream_t stream) {
    if (!W || !colsum_ws || Nin <= 0 || N <= 0 || (w_dtype != kWF16 && w_dtype != kWBF16)) return SNN_ERR_INVALID;
    if (Nin > kMaxTerms) return SNN_ERR_UNSUPPORTED;
    const long E = (long)Nin * N;
    const unsigned gf = (unsigned)((N + 63) / 64), gs = (unsigned)((E + 255) / 256 < 4096 ? (E + 255) / 256 : 4096);
    hipStream_t st = (hipStream_t)stream;
    if (w_dtype == kWF16) {
        hipLaunchKernelGGL(k_norm_factor_h16<kWF16>, dim3(gf), dim3(64), 0, st, (const uint16_t *)W, Nin, N, norm, colsum_ws);
        hipLaunchKernelGGL(k_norm_scale_h16<kWF16>, dim3(gs), dim3(256), 0, st, (uint16_t *)W, E, N, colsum_ws);
    } else {
        hipLaunchKernelGGL(k_norm_factor_h16<kWBF16>, dim3(gf), dim3(64), 0, st, (const uint16_t *)W, Nin, N, norm, colsum_ws);
        hipLaunchKernelGGL(k_norm_scale_h16<kWBF16>, dim3(gs), dim3(256), 0, st, (uint16_t *)W, E, N, colsum_ws);
    }
    return snn_check_launch();
}
