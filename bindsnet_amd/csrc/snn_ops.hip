// snn_ops.hip -- per-operator gfx950 kernels + their C-ABI entry points (include/snnhip.h).
// One entry point per reference function of SURVEY.md 8(a); the fused multi-step drivers live in
// snn_run.hip and reuse the device code here.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see csrc/Makefile).  -ffp-contract=off
// is load-bearing: the reference rounds after every multiply and every add.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/snnhip.h"
#include "snn_conv_events.hpp"
#include "snn_order.hpp"
#include "snn_conv_apply.hpp"
#include "snn_common.hpp"
#include "snn_rng.hpp"
#include "snn_synparams.hpp"

using namespace snn;

// =============================================================================================
// a5 / a6: spike propagation, event-driven.
// grid (ceil(N/256), B), 256 threads: thread <-> target column j, block <-> sample b.
// Per 1024-source chunk each of the 4 waves compacts its 256 sources into an ascending list in
// LDS (wave ballot + popcount), then every thread walks the 4 lists in order and accumulates
// W[i,j] (coalesced 1 KiB row segments) through the ordered-sum state machine.
// =============================================================================================
template <class SUM>
__device__ __forceinline__ void prop_body(const float *__restrict__ W, const float *__restrict__ bias,
                                          const uint8_t *__restrict__ s, float *__restrict__ out,
                                          int B, int Nin, int N, int accumulate) {
    __shared__ uint32_t list[4][256];
    __shared__ int cnt[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y, j = blockIdx.x * 256 + tid;
    const bool valid = j < N;
    const int jc = valid ? j : N - 1;
    const uint8_t *srow = s + (size_t)b * Nin;
    SUM acc;
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
                uint32_t e[4]; float wv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    e[u] = list[w][(k + u < n) ? k + u : k];
                    wv[u] = W[(size_t)(e[u] >> 8) * N + jc];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + u < n) acc.add((int)(e[u] >> 8), wv[u] * (float)(e[u] & 255u), Nin);
            }
        }
        __syncthreads();
    }
    if (valid) {
        float r = acc.finish(Nin);
        if (bias) r = r + bias[j];
        const size_t o = (size_t)b * N + j;
        out[o] = (accumulate ? out[o] : 0.0f) + r;
    }
}

template <class SUM>
__global__ __launch_bounds__(256) void k_prop(const float *__restrict__ W, const float *__restrict__ bias,
                                              const uint8_t *__restrict__ s, float *__restrict__ out,
                                              int B, int Nin, int N, int accumulate) {
    prop_body<SUM>(W, bias, s, out, B, Nin, N, accumulate);
}

// The second launch of snn_prop_dense_auto_f32 (csrc/snn_mfma.hip): the same body, but the workgroups of a sample whose tile of 16
// the matrix kernel has stored (flags[b / 16] != 0, written by the launch before this one) return at once.
__global__ __launch_bounds__(256) void k_prop_flagged(const float *__restrict__ W, const float *__restrict__ bias,
                                                      const uint8_t *__restrict__ s, float *__restrict__ out,
                                                      int B, int Nin, int N, int accumulate, const int *__restrict__ flags) {
    if (flags[blockIdx.y >> 4]) return;                 // (uniform)
    prop_body<SeqSum>(W, bias, s, out, B, Nin, N, accumulate);
}

// N == 1: the reference's sum over the sources of ONE contiguous column is ATen's inner reduction (snn_order.hpp inner_sum8_terms),
// not an outer sum.  One thread per sample; a layer of one neuron is no hot path.
__global__ __launch_bounds__(64) void k_prop_col1(const float *__restrict__ W, const uint8_t *__restrict__ s, float *__restrict__ out,
                                                  int B, int Nin, int accumulate) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const uint8_t *srow = s + (size_t)b * Nin;
    const float r = inner_sum8_terms([=](int i) { return W[i] * (float)srow[i]; }, Nin);
    out[b] = (accumulate ? out[b] : 0.0f) + r;
}

extern "C" int snn_prop_cascade_f32(const float *W, const uint8_t *s, float *out, int B, int Nin, int N,
                                    int accumulate, snn_stream_t stream) {
    if (!W || !s || !out || B <= 0 || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (Nin > kMaxTerms || B > 65535) return SNN_ERR_UNSUPPORTED;
    if (N == 1) {
        hipLaunchKernelGGL(k_prop_col1, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, W, s, out, B, Nin, accumulate);
        return snn_check_launch();
    }
    hipLaunchKernelGGL(k_prop<OuterSum>, dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, W,
                       (const float *)nullptr, s, out, B, Nin, N, accumulate);
    return snn_check_launch();
}

extern "C" int snn_prop_dense_f32(const float *W, const float *bias, const uint8_t *s, float *out, int B,
                                  int Nin, int N, int accumulate, snn_stream_t stream) {
    if (!W || !s || !out || B <= 0 || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (Nin >= (1 << 24) || B > 65535) return SNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_prop<SeqSum>, dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, W, bias, s,
                       out, B, Nin, N, accumulate);
    return snn_check_launch();
}

int snn_launch_prop_dense_flagged(const float *W, const float *bias, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate,
                                  const int *flags, hipStream_t stream) {
    hipLaunchKernelGGL(k_prop_flagged, dim3((N + 255) / 256, B), dim3(256), 0, stream, W, bias, s, out, B, Nin, N, accumulate, flags);
    return snn_check_launch();
}

// =============================================================================================
// a7: conv2d propagation.  thread <-> (b, oy, ox, chunk of 8 output channels) -- blockIdx.y = the chunk (round 6: with all channels of a
// pixel on one thread the conv_mnist.py shapes gave 36 workgroups and 58 us per call; 8 us like this); weights broadcast from LDS.
// Tap order (kh, kw, cin): taps row-major, input channels innermost (what oneDNN does for C_in <= 16), sequential, + bias.
// =============================================================================================
__global__ __launch_bounds__(256) void k_conv2d(const float *__restrict__ W, const float *__restrict__ bias,
                                                const uint8_t *__restrict__ s, float *__restrict__ out, int B,
                                                int Cin, int H, int Wd, int Cout, int KH, int KW, int stride,
                                                int pad, int OH, int OW, int accumulate, int nstage) {
    extern __shared__ float wsm[];  // [Cout][Cin*KH*KW] | staged input images of the block's samples (u8, when they fit: nstage > 0)
    const int taps = Cin * KH * KW;
    for (int k = threadIdx.x; k < Cout * taps; k += blockDim.x) wsm[k] = W[k];
    const long npix = (long)B * OH * OW;
    const long p0 = (long)blockIdx.x * blockDim.x;
    const int img = Cin * H * Wd, bfirst = (int)(p0 / ((long)OW * OH));
    uint8_t *simg = (uint8_t *)(wsm + Cout * taps);
    if (nstage > 0) {                                    // the images of samples bfirst .. bfirst + nstage - 1: every window of the block reads them
        const long n = (long)min(nstage, B - bfirst) * img;
        const uint8_t *src = s + (size_t)bfirst * img;
        for (long k = threadIdx.x; k < n; k += blockDim.x) simg[k] = src[k];
    }
    __syncthreads();
    const long p = p0 + threadIdx.x;
    if (p >= npix) return;
    const int ox = (int)(p % OW), oy = (int)((p / OW) % OH), b = (int)(p / ((long)OW * OH));
    const uint8_t *sb = nstage > 0 ? simg + (size_t)(b - bfirst) * img : s + (size_t)b * img;
    {
        const int c0 = (int)blockIdx.y * 8;
        float acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = 0.f;
        for (int ky = 0; ky < KH; ++ky)               // reference order: taps row-major, input channels innermost
            for (int kx = 0; kx < KW; ++kx)
                for (int ci = 0; ci < Cin; ++ci) {
                    const int tap = (ci * KH + ky) * KW + kx;
                    const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
                    if (iy < 0 || iy >= H || ix < 0 || ix >= Wd) continue;
                    const uint8_t sv = sb[((size_t)ci * H + iy) * Wd + ix];
                    if (!sv) continue;
                    const float fs = (float)sv;
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (c0 + u < Cout) acc[u] += fs * wsm[(c0 + u) * taps + tap];
                }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (c0 + u < Cout) {
                float r = acc[u];
                if (bias) r = r + bias[c0 + u];
                const size_t o = (((size_t)b * Cout + c0 + u) * OH + oy) * OW + ox;
                out[o] = (accumulate ? out[o] : 0.0f) + r;
            }
    }
}

int snn_conv_wide_launch(const float *W, const float *bias, const uint8_t *s, float *out, int B, int Cin, int H, int Wd, int Cout,
                         int KH, int KW, int stride, int pad, int OH, int OW, int accumulate, hipStream_t stream);      // snn_conv_wide.hip

extern "C" int snn_prop_conv2d_f32(const float *W, const float *bias, const uint8_t *s, float *out, int B,
                                   int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad,
                                   int accumulate, snn_stream_t stream) {
    if (!W || !s || !out || B <= 0 || Cin <= 0 || H <= 0 || Wd <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 ||
        stride <= 0 || pad < 0)
        return SNN_ERR_INVALID;
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (Wd + 2 * pad - KW) / stride + 1;
    if (OH <= 0 || OW <= 0) return SNN_ERR_INVALID;
    size_t lds = sizeof(float) * (size_t)Cout * Cin * KH * KW;
    if (Cin > 16 || lds > 64 * 1024)               // more channels than k_conv2d was written for, or a bank beyond its LDS: the same order, slab by slab (snn_conv_wide.hip)
        return snn_conv_wide_launch(W, bias, s, out, B, Cin, H, Wd, Cout, KH, KW, stride, pad, OH, OW, accumulate, (hipStream_t)stream);
    const long npix = (long)B * OH * OW;
    // a block of 256 consecutive output pixels touches at most 255 / (OH * OW) + 2 samples: their input images go to LDS when they fit 32 KB
    int nstage = 255 / (OH * OW) + 2;
    if ((size_t)nstage * Cin * H * Wd > 32 * 1024) nstage = 0; else lds += (size_t)nstage * Cin * H * Wd;
    static bool attr_set = false;
    if (!attr_set) {   // a 64 KiB bank and 32 KiB of staged images: up to 96 KiB of dynamic LDS
        if (snn_check(hipFuncSetAttribute((const void *)k_conv2d, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024))) return SNN_ERR_LAUNCH;
        attr_set = true;
    }
    hipLaunchKernelGGL(k_conv2d, dim3((unsigned)((npix + 255) / 256), (unsigned)((Cout + 7) / 8)), dim3(256), lds, (hipStream_t)stream, W,
                       bias, s, out, B, Cin, H, Wd, Cout, KH, KW, stride, pad, OH, OW, accumulate, nstage);
    return snn_check_launch();
}

// =============================================================================================
// a2: input layer: trace + raster.
// =============================================================================================
__global__ __launch_bounds__(256) void k_input(const uint8_t *__restrict__ s, float *__restrict__ x, long n,
                                               float trace_decay, float trace_scale, int additive,
                                               uint8_t *__restrict__ raster) {
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x) {
        const uint8_t sv = s[k];
        if (x) x[k] = trace_next(x[k], sv, trace_decay, trace_scale, additive);
        if (raster) raster[k] = sv;
    }
}

// The same with per-neuron trace constants (snn_pervec: trace_decay[j], and trace_scale[j] with additive traces): the grid is
// (blocks over the N neurons, B samples), as in every per-neuron instance -- row j is loaded without a division.
__global__ __launch_bounds__(256) void k_input_pv(const uint8_t *__restrict__ s, float *__restrict__ x, int N, snn_lif_params p,
                                                  snn_pervec pv, uint8_t *__restrict__ raster) {
    const long base = (long)blockIdx.y * N;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (long)gridDim.x * blockDim.x) {
        const long k = base + j;
        const node_row r = row_of<true>(p, 0.f, pv, j);
        const uint8_t sv = s[k];
        if (x) x[k] = trace_next(x[k], sv, r.trace_decay, r.trace_scale, p.traces_additive);
        if (raster) raster[k] = sv;
    }
}

extern "C" int snn_input_step(const uint8_t *s, float *x, long n_total, float trace_decay, float trace_scale,
                              int additive, uint8_t *raster_out, snn_stream_t stream);
extern "C" int snn_input_step_pv(const uint8_t *s, float *x, int B, int N, float trace_decay, float trace_scale, int additive,
                                 const snn_pervec *pv, uint8_t *raster_out, snn_stream_t stream) {
    if (B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (!pervec_any(pv)) return snn_input_step(s, x, (long)B * N, trace_decay, trace_scale, additive, raster_out, stream);
    if (!s || !x) return SNN_ERR_INVALID;
    if (!pervec_within(pv, kPvTrace) || (pv->v[SNN_PV_TRACE_SCALE] && !additive)) return SNN_ERR_INVALID;
    if (B > 65535) return SNN_ERR_UNSUPPORTED;
    snn_lif_params p = {};
    p.traces = 1; p.trace_decay = trace_decay; p.trace_scale = trace_scale; p.traces_additive = additive;
    const unsigned gx = (unsigned)((N + 255) / 256 < 2048 ? (N + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_input_pv, dim3(gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, s, x, N, p, *pv, raster_out);
    return snn_check_launch();
}

extern "C" int snn_input_step(const uint8_t *s, float *x, long n_total, float trace_decay, float trace_scale,
                              int additive, uint8_t *raster_out, snn_stream_t stream) {
    if (!s || n_total <= 0) return SNN_ERR_INVALID;
    if (!x && !raster_out) return SNN_OK;
    const unsigned grid = (unsigned)((n_total + 255) / 256 < 2048 ? (n_total + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_input, dim3(grid), dim3(256), 0, (hipStream_t)stream, s, x, n_total, trace_decay,
                       trace_scale, additive, raster_out);
    return snn_check_launch();
}

// =============================================================================================
// a3: LIF step, fully elementwise (state streaming: v, refrac r/w, I r/w, s w, x r/w).
// =============================================================================================
template <bool VTH>
__global__ __launch_bounds__(256) void k_lif(float *__restrict__ v, float *__restrict__ refrac,
                                             uint8_t *__restrict__ s, float *__restrict__ x,
                                             float *__restrict__ I, long n, snn_lif_params p,
                                             uint8_t *__restrict__ raster_s, float *__restrict__ raster_v,
                                             const float *__restrict__ thresh_vec, int N) {
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x) {
        float vv = v[k], rc = refrac[k], cur = I[k];
        if (rc > 0.f) { cur = 0.f; I[k] = 0.f; }   // nodes.py:511 masks the caller's tensor in place
        if (VTH) p.thresh = thresh_vec[k % N];     // nodes.py:519 with a tensor-valued `thresh`: broadcast over the batch
        const uint8_t sp = lif_update(vv, rc, cur, p);
        v[k] = vv; refrac[k] = rc; s[k] = sp;
        if (p.traces) x[k] = trace_next(x[k], sp, p.trace_decay, p.trace_scale, p.traces_additive);
        if (raster_s) raster_s[k] = sp;
        if (raster_v) raster_v[k] = vv;
    }
}

// k_lif with per-neuron parameters (snn_pervec: thresh[j], decay[j], trace_decay[j], trace_scale[j]).  Grid (blocks over the N
// neurons, B samples): the loop carries the neuron j of sample blockIdx.y, so the [N] rows are loaded coalesced and without the
// division of the VTH instance above; the B blocks of a column range find them in L2.
__global__ __launch_bounds__(256) void k_lif_pv(float *__restrict__ v, float *__restrict__ refrac, uint8_t *__restrict__ s,
                                                float *__restrict__ x, float *__restrict__ I, int N, snn_lif_params p,
                                                uint8_t *__restrict__ raster_s, float *__restrict__ raster_v, snn_pervec pv) {
    const long base = (long)blockIdx.y * N;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (long)gridDim.x * blockDim.x) {
        const long k = base + j;
        const node_row r = row_of<true>(p, 0.f, pv, j);
        float vv = v[k], rc = refrac[k], cur = I[k];
        if (rc > 0.f) { cur = 0.f; I[k] = 0.f; }   // nodes.py:511 masks the caller's tensor in place
        const uint8_t sp = lif_update(vv, rc, cur, p, r.thresh, r.decay);
        v[k] = vv; refrac[k] = rc; s[k] = sp;
        if (p.traces) x[k] = trace_next(x[k], sp, r.trace_decay, r.trace_scale, p.traces_additive);
        if (raster_s) raster_s[k] = sp;
        if (raster_v) raster_v[k] = vv;
    }
}

extern "C" int snn_lif_step(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N,
                            const snn_lif_params *h_p, uint8_t *raster_s, float *raster_v, snn_stream_t stream);
extern "C" int snn_lif_step_pv(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N, const snn_lif_params *h_p,
                               const snn_pervec *pv, uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    if (!pervec_any(pv)) return snn_lif_step(v, refrac, s, x, I, B, N, h_p, raster_s, raster_v, stream);
    if (!v || !refrac || !s || !I || !h_p || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (h_p->traces && !x) return SNN_ERR_INVALID;
    if (!pervec_within(pv, kPvThresh | kPvDecay | kPvTrace) || (pv->v[SNN_PV_TRACE_SCALE] && !h_p->traces_additive)) return SNN_ERR_INVALID;
    if (B > 65535) return SNN_ERR_UNSUPPORTED;
    const unsigned gx = (unsigned)((N + 255) / 256 < 4096 ? (N + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_lif_pv, dim3(gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, v, refrac, s, x, I, N, *h_p, raster_s, raster_v, *pv);
    return snn_check_launch();
}

extern "C" int snn_lif_step_vth(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N,
                                const snn_lif_params *h_p, const float *thresh_vec, uint8_t *raster_s, float *raster_v,
                                snn_stream_t stream) {
    if (!v || !refrac || !s || !I || !h_p || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (h_p->traces && !x) return SNN_ERR_INVALID;
    const long n = (long)B * N;
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    if (thresh_vec)
        hipLaunchKernelGGL(k_lif<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, v, refrac, s, x, I, n, *h_p,
                           raster_s, raster_v, thresh_vec, N);
    else
        hipLaunchKernelGGL(k_lif<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, v, refrac, s, x, I, n, *h_p,
                           raster_s, raster_v, thresh_vec, N);
    return snn_check_launch();
}

extern "C" int snn_lif_step(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N,
                            const snn_lif_params *h_p, uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    return snn_lif_step_vth(v, refrac, s, x, I, B, N, h_p, nullptr, raster_s, raster_v, stream);
}

// =============================================================================================
// a4: Diehl&Cook step = two kernels.
//  k_dc_membrane: thread <-> neuron j, loops the batch (theta is shared by the batch and needs the
//                 per-neuron spike count over b) -> crossings written to s; snapshots the cursor.
//  k_dc_arbitrate: block <-> sample b: rank of b among rows with a crossing (noise offset),
//                 argmax of 1/q over the candidates (first maximal index), winner written back,
//                 trace + raster for the row.  The block of the last row publishes the new cursor.
// =============================================================================================
// PV (both kernels): the instance for per-neuron parameters (snn_pervec).  Thread <-> neuron j here, so row j -- thresh[j],
// decay[j], theta_decay[j], theta_plus[j] -- is loaded once, beside theta[j], for the whole batch.
template <bool PV>
__global__ __launch_bounds__(256) void k_dc_membrane(float *__restrict__ v, float *__restrict__ refrac,
                                                     uint8_t *__restrict__ s, float *__restrict__ theta,
                                                     const float *__restrict__ I, int B, int N,
                                                     snn_dc_params p, long long *__restrict__ cursor,
                                                     float *__restrict__ raster_v, snn_pervec pv) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0 && cursor) cursor[1] = cursor[0];   // snapshot read by k_dc_arbitrate
    if (j >= N) return;
    const node_row r = row_of<PV>(p, 0.f, pv, j);
    const float th0 = dc_theta_decayed(theta[j], p.learning, r.theta_decay);   // nodes.py:1079
    const float thr = r.thresh + th0;                   // nodes.py:1088
    int cnt = 0;
    for (int b = 0; b < B; ++b) {
        const size_t k = (size_t)b * N + j;
        float vv = v[k], rc = refrac[k];
        const uint8_t sp = dc_update(vv, rc, I[k], thr, p.lif, r.decay);
        v[k] = vv; refrac[k] = rc; s[k] = sp;
        cnt += sp;
        if (raster_v) raster_v[k] = vv;
    }
    theta[j] = dc_theta_bumped(th0, p.learning, r.theta_plus, cnt);            // nodes.py:1094 (count is exact in f32)
}

template <bool PV>
__global__ __launch_bounds__(256) void k_dc_arbitrate(uint8_t *__restrict__ s, float *__restrict__ x, int B,
                                                      int N, snn_dc_params p, const float *__restrict__ Q,
                                                      long long q_len, long long *__restrict__ cursor,
                                                      int *__restrict__ status, uint8_t *__restrict__ raster_s, snn_pervec pv) {
    __shared__ int any_row[1024];
    __shared__ float red_v[4];
    __shared__ int red_j[4];
    __shared__ int s_win;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
    int win = -2;  // -2: keep crossings as they are (one_spike off / no crossing / noise exhausted)
    if (p.one_spike) {
        // which rows 0..b have a crossing: one wave per row, strided
        for (int r = wave; r <= b; r += 4) {
            bool a = false;
            for (int j = lane; j < N; j += 64) a |= s[(size_t)r * N + j] != 0;
            const uint64_t m = __ballot(a);
            if (lane == 0) any_row[r] = m != 0;
        }
        __syncthreads();
        int rank = 0;
        for (int r = 0; r < b; ++r) rank += any_row[r];
        const int mine = any_row[b];
        const long long cur = cursor[1];
        const long long off = cur + (long long)rank * N;
        if (b == B - 1) {
            const long long nxt = cur + (long long)(rank + mine) * N;
            if (tid == 0) { cursor[0] = nxt <= q_len ? nxt : cur; if (nxt > q_len) atomicExch(status, SNN_ERR_NOISE); }
        }
        if (mine && off + N <= q_len) {
            float bv = -1.f; int bj = 0x7fffffff;
            for (int j = tid; j < N; j += 256)
                if (s[(size_t)b * N + j]) {
                    const float val = 1.0f / Q[off + j];        // p / q with p = 1 (nodes.py:1100-1102)
                    if (val > bv) { bv = val; bj = j; }         // ascending j: strict > keeps the first max
                }
            // wave reduce: max value, ties -> lowest index
            for (int d = 32; d >= 1; d >>= 1) {
                const float ov = __shfl_xor(bv, d); const int oj = __shfl_xor(bj, d);
                if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
            }
            if (lane == 0) { red_v[wave] = bv; red_j[wave] = bj; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < 4; ++w)
                    if (red_v[w] > bv || (red_v[w] == bv && red_j[w] < bj)) { bv = red_v[w]; bj = red_j[w]; }
                s_win = bj;
            }
            __syncthreads();
            win = s_win;
        } else if (mine) {
            if (tid == 0) atomicExch(status, SNN_ERR_NOISE);
        }
    }
    for (int j = tid; j < N; j += 256) {
        const size_t k = (size_t)b * N + j;
        uint8_t sp = s[k];
        if (win >= 0) { sp = (j == win); s[k] = sp; }
        if (p.lif.traces) {
            const node_row r = row_of<PV>(p, 0.f, pv, j);
            x[k] = trace_next(x[k], sp, r.trace_decay, r.trace_scale, p.lif.traces_additive);
        }
        if (raster_s) raster_s[k] = sp;
    }
}

// `pv`: nullable; the vectors a Diehl&Cook / AdaptiveLIF layer reads (anything else was refused by the caller)
int snn_launch_dc_membrane(float *v, float *refrac, uint8_t *s, float *theta, const float *I, int B, int N,
                           const snn_dc_params &p, long long *cursor, float *raster_v, hipStream_t st, const snn_pervec *pv) {
    if (pervec_any(pv))
        hipLaunchKernelGGL(k_dc_membrane<true>, dim3((N + 255) / 256), dim3(256), 0, st, v, refrac, s, theta, I, B, N, p, cursor,
                           raster_v, *pv);
    else
        hipLaunchKernelGGL(k_dc_membrane<false>, dim3((N + 255) / 256), dim3(256), 0, st, v, refrac, s, theta, I, B, N, p, cursor,
                           raster_v, snn_pervec{});
    return snn_check_launch();
}

int snn_launch_dc_arbitrate(uint8_t *s, float *x, int B, int N, const snn_dc_params &p, const float *Q, long long q_len,
                            long long *cursor, int *status, uint8_t *raster_s, hipStream_t st, const snn_pervec *pv) {
    if (pv && (pv->v[SNN_PV_TRACE_DECAY] || pv->v[SNN_PV_TRACE_SCALE]))
        hipLaunchKernelGGL(k_dc_arbitrate<true>, dim3(B), dim3(256), 0, st, s, x, B, N, p, Q, q_len, cursor, status, raster_s, *pv);
    else
        hipLaunchKernelGGL(k_dc_arbitrate<false>, dim3(B), dim3(256), 0, st, s, x, B, N, p, Q, q_len, cursor, status, raster_s,
                           snn_pervec{});
    return snn_check_launch();
}

static bool pervec_dc_ok(const snn_pervec *pv, const snn_dc_params &p) {
    return pervec_within(pv, kPvThresh | kPvDecay | kPvTrace | kPvTheta) && !(pv && pv->v[SNN_PV_TRACE_SCALE] && !p.lif.traces_additive);
}

extern "C" int snn_dc_step_pv(float *v, float *refrac, uint8_t *s, float *x, float *theta, const float *I, int B, int N,
                              const snn_dc_params *h_p, const snn_pervec *pv, const float *noise_q, long long q_len,
                              long long *cursor, int *status, uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    if (!v || !refrac || !s || !theta || !I || !h_p || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (h_p->lif.traces && !x) return SNN_ERR_INVALID;
    if (h_p->one_spike && (!noise_q || !cursor || !status)) return SNN_ERR_INVALID;
    if (!pervec_dc_ok(pv, *h_p)) return SNN_ERR_INVALID;
    if (B > 1024) return SNN_ERR_UNSUPPORTED;
    int rc = snn_launch_dc_membrane(v, refrac, s, theta, I, B, N, *h_p, cursor, raster_v, (hipStream_t)stream, pv);
    if (rc) return rc;
    return snn_launch_dc_arbitrate(s, x, B, N, *h_p, noise_q, q_len, cursor, status, raster_s, (hipStream_t)stream, pv);
}

extern "C" int snn_dc_step(float *v, float *refrac, uint8_t *s, float *x, float *theta, const float *I, int B,
                           int N, const snn_dc_params *h_p, const float *noise_q, long long q_len,
                           long long *cursor, int *status, uint8_t *raster_s, float *raster_v,
                           snn_stream_t stream) {
    return snn_dc_step_pv(v, refrac, s, x, theta, I, B, N, h_p, nullptr, noise_q, q_len, cursor, status, raster_s, raster_v, stream);
}

extern "C" int snn_dc_arbitrate(uint8_t *s, float *x, int B, int N, const snn_dc_params *h_p, const float *noise_q,
                                long long q_len, long long *cursor, int *status, uint8_t *raster_s,
                                snn_stream_t stream) {
    if (!s || !h_p || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (h_p->lif.traces && !x) return SNN_ERR_INVALID;
    if (h_p->one_spike && (!noise_q || !cursor || !status)) return SNN_ERR_INVALID;
    if (B > 1024) return SNN_ERR_UNSUPPORTED;
    return snn_launch_dc_arbitrate(s, x, B, N, *h_p, noise_q, q_len, cursor, status, raster_s, (hipStream_t)stream, nullptr);
}

// ---------------------------------------------------------------------------------------------
// Device-side noise for one_spike: materialise, for the rows that crossed threshold this step,
// exactly the Exp(1) draws torch.multinomial would consume (row-major over [rows_with_crossing, N]),
// but only at the candidate positions (the others are never read by the arbitration).
// One workgroup: the mt19937 state is staged in LDS and advanced block by block.
// qbuf[rank*N + j] receives the draw of candidate (b, j); cursor[1] is zeroed so that
// k_dc_arbitrate indexes qbuf from 0.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_rng_fill(snn_rng_state *__restrict__ rng, const uint8_t *__restrict__ s,
                                                   int B, int N, float *__restrict__ qbuf,
                                                   long long *__restrict__ cursor) {
    __shared__ uint32_t mt[2][624];
    __shared__ int rank[1025];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < 624; i += 1024) mt[0][i] = rng->mt[i];
    for (int r = wave; r < B; r += 16) {
        bool a = false;
        for (int j = lane; j < N; j += 64) a |= s[(size_t)r * N + j] != 0;
        const uint64_t m = __ballot(a);
        if (lane == 0) rank[r + 1] = m != 0;
    }
    __syncthreads();
    if (tid == 0) {
        rank[0] = 0;
        for (int r = 0; r < B; ++r) rank[r + 1] += rank[r];
        cursor[1] = 0;
    }
    __syncthreads();
    const int rows = rank[B];
    if (rows == 0) return;
    const long long pos = rng->pos;
    const long long E = pos + 2ll * rows * N;          // one past the last 32-bit output consumed
    const int ntw = (int)((E - 1) / 624);              // twists the lazy generator performs
    const long long total = (long long)B * N;
    for (int m = 0; m <= ntw; ++m) {
        const uint32_t *cur = mt[m & 1];
        for (long long idx = tid; idx < total; idx += 1024) {
            if (!s[idx]) continue;
            const int b = (int)(idx / N), j = (int)(idx - (long long)b * N);
            if (rank[b + 1] == rank[b]) continue;
            const long long d = (long long)rank[b] * N + j;
            const long long w0 = pos + 2 * d, w1 = w0 + 1;
            const int m0 = (int)(w0 / 624), m1 = (int)(w1 / 624);
            if (m0 == m && m1 == m) {
                qbuf[d] = exp1_from_words(mt_temper(cur[w0 - 624ll * m]), mt_temper(cur[w1 - 624ll * m]));
            } else if (m0 == m) {                        // pair straddles a twist: park the high word
                qbuf[d] = __uint_as_float(mt_temper(cur[w0 - 624ll * m]));
            } else if (m1 == m) {
                qbuf[d] = exp1_from_words(__float_as_uint(qbuf[d]), mt_temper(cur[w1 - 624ll * m]));
            }
        }
        __syncthreads();
        if (m < ntw) mt_twist_block(mt[m & 1], mt[(m + 1) & 1], tid, 1024);
    }
    for (int i = tid; i < 624; i += 1024) rng->mt[i] = mt[ntw & 1][i];
    if (tid == 0) {
        rng->pos = (int)(E - 624ll * ntw);
        rng->consumed += (long long)rows * N;
    }
}

int snn_launch_rng_fill(snn_rng_state *rng, const uint8_t *s, int B, int N, float *qbuf, long long *cursor,
                        hipStream_t st) {
    hipLaunchKernelGGL(k_rng_fill, dim3(1), dim3(1024), 0, st, rng, s, B, N, qbuf, cursor);
    return snn_check_launch();
}

extern "C" int snn_rng_fill_exponential(snn_rng_state *rng, const uint8_t *crossings, int B, int N, float *qbuf,
                                        long long *cursor, snn_stream_t stream) {
    if (!rng || !crossings || !qbuf || !cursor || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (B > 1024) return SNN_ERR_UNSUPPORTED;
    return snn_launch_rng_fill(rng, crossings, B, N, qbuf, cursor, (hipStream_t)stream);
}

// =============================================================================================
// a8 / a9 / a10: outer-product plasticity.  grid (ceil(N/TJ), ceil(Nin/16)), 256 threads.
// A block owns a 16 x TJ tile of W.  The batch-side factors of the tile's rows and columns are
// staged in LDS once; per element the batch reduction walks only the samples in which the row's
// source or the column's target spiked (bit masks over b), through the ATen-ordered accumulator.
// =============================================================================================
struct StdpArgs {
    float *W;
    const uint8_t *s_src; const float *x_src; const uint8_t *s_tgt; const float *x_tgt;
    int B, Nin, N;
    float nu0, nu1; int use_dt; float dt, decay;
    int has_min; float wmin; int has_max; float wmax;
    int assume_clamped;
    // MSTDP (mode 1): x_src = p_plus, x_tgt = p_minus, s_* = previous-step spikes
    // mode 2: Hebbian (learning.py:1110-1135), mode 3: WeightDependentPostPre (learning.py:626-653): raw outer products
    // reduced over the batch first, learning rates (and the weight-dependent factors) applied to the sums
    int mode; float reward; const float *reward_vec;
};

constexpr int kTI = 16;

// k_plasticity<TJ> (scalar rates and bounds) and k_plasticity_pv<TJ> (per-synapse: snn_synparams) are one text compiled twice
#define SNN_PLASTICITY_PV 0
#include "snn_plasticity.inc"
#undef SNN_PLASTICITY_PV
#define SNN_PLASTICITY_PV 1
#include "snn_plasticity.inc"
#undef SNN_PLASTICITY_PV
// ... and a third time as k_plasticity_red<TJ, ACC>: the batch reductions beside sum (snnhip.h f15)
#define SNN_PLASTICITY_PV 2
#include "snn_plasticity.inc"
#undef SNN_PLASTICITY_PV

// One launcher for the three inclusions of the kernel text: the LDS formula, the tile thresholds and the > 64 KiB attribute of the
// narrow-tile instance are in one place.  FAMILY names the four tile instances; `extra` is what the kernel takes behind StdpArgs.
struct PlasticityScalar {                              // k_plasticity<TJ>(StdpArgs)
    template <int TJ> static auto kernel() { return k_plasticity<TJ>; }
};
struct PlasticityPv {                                  // k_plasticity_pv<TJ>(StdpArgs, snn_synparams)
    template <int TJ> static auto kernel() { return k_plasticity_pv<TJ>; }
};
template <int R> struct PlasticityRed {                // k_plasticity_red<TJ, BatchReduce<R>>(StdpArgs, snn_synparams)
    template <int TJ> static auto kernel() { return k_plasticity_red<TJ, BatchReduce<R>>; }
};

template <class FAMILY, class... EXTRA>
static int launch_plasticity_tiles(const StdpArgs &a, hipStream_t st, const EXTRA &...extra) {
    const int B = a.B, MW = (B + 31) / 32;
    auto lds = [&](int TJ) {
        return (size_t)B * TJ * 4 + (size_t)B * kTI * 4 + (size_t)(TJ + kTI) * MW * 4 + (size_t)B * TJ + (size_t)B * kTI;
    };
    const dim3 blk(256);
    const unsigned gy = (a.Nin + kTI - 1) / kTI;
    constexpr size_t kSmall = 64 * 1024, kBig = 144 * 1024;   // 160 KiB LDS per CU on gfx950
    static bool attr_set = false;                      // (one per FAMILY)
    if (!attr_set) {   // allow > 64 KiB dynamic LDS for the narrow-tile instantiation
        if (snn_check(hipFuncSetAttribute((const void *)FAMILY::template kernel<32>(), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)kBig)))
            return SNN_ERR_LAUNCH;
        attr_set = true;
    }
    if (lds(256) <= kSmall) {
        hipLaunchKernelGGL(FAMILY::template kernel<256>(), dim3((a.N + 255) / 256, gy), blk, lds(256), st, a, extra...);
    } else if (lds(128) <= kSmall) {
        hipLaunchKernelGGL(FAMILY::template kernel<128>(), dim3((a.N + 127) / 128, gy), blk, lds(128), st, a, extra...);
    } else if (lds(64) <= kSmall) {
        hipLaunchKernelGGL(FAMILY::template kernel<64>(), dim3((a.N + 63) / 64, gy), blk, lds(64), st, a, extra...);
    } else if (lds(32) <= kBig) {
        hipLaunchKernelGGL(FAMILY::template kernel<32>(), dim3((a.N + 31) / 32, gy), blk, lds(32), st, a, extra...);
    } else {
        return SNN_ERR_UNSUPPORTED;
    }
    return snn_check_launch();
}

static int launch_plasticity(const StdpArgs &a, hipStream_t st) { return launch_plasticity_tiles<PlasticityScalar>(a, st); }

// The same tiles and LDS layout for the per-synapse instance (k_plasticity_pv) ...
static int launch_plasticity_pv(const StdpArgs &a, const snn_synparams &q, hipStream_t st) {
    return launch_plasticity_tiles<PlasticityPv>(a, st, q);
}

static bool reduce_valid(int reduce) { return reduce >= SNN_REDUCE_SUM && reduce <= SNN_REDUCE_AMIN; }

// ... and for the instances of another batch reduction (k_plasticity_red<TJ, BatchReduce<R>>).
// `reduce` is MEAN, AMAX or AMIN here (SUM is the two instances above: launch_plasticity_for); a NULL `sp` is the empty snn_synparams.
static int launch_plasticity_red(const StdpArgs &a, const snn_synparams &q, int reduce, hipStream_t st) {
    switch (reduce) {
        case SNN_REDUCE_MEAN: return launch_plasticity_tiles<PlasticityRed<SNN_REDUCE_MEAN>>(a, st, q);
        case SNN_REDUCE_AMAX: return launch_plasticity_tiles<PlasticityRed<SNN_REDUCE_AMAX>>(a, st, q);
        case SNN_REDUCE_AMIN: return launch_plasticity_tiles<PlasticityRed<SNN_REDUCE_AMIN>>(a, st, q);
        default: return SNN_ERR_INVALID;
    }
}

// The scalar fields of StdpArgs for the per-synapse instance: a rate given as a tensor leaves "any entry non-zero" in its place.
static void syn_rates(StdpArgs &a, const snn_synparams &q) {
    if (q.nu0) a.nu0 = q.nu0_any ? 1.f : 0.f;
    if (q.nu1) a.nu1 = q.nu1_any ? 1.f : 0.f;
}

// The instance of an update, chosen once per rule body: another batch reduction -> k_plasticity_red; per-synapse constants ->
// k_plasticity_pv; else the scalar kernel, which never looks at `sp`.
static int launch_plasticity_for(const StdpArgs &a, const snn_synparams *sp, int reduce, hipStream_t st) {
    if (reduce != SNN_REDUCE_SUM) return launch_plasticity_red(a, sp ? *sp : snn_synparams{}, reduce, st);
    return syn_any(sp) ? launch_plasticity_pv(a, *sp, st) : launch_plasticity(a, st);
}

// a8 / a9: PostPre.  The scalar name passes sp = NULL and SUM, the *_pv name SUM.
static int postpre_dense(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Nin, int N,
                         float nu0, float nu1, int use_dt, float dt, float decay, int has_min, float wmin, int has_max, float wmax,
                         int assume_clamped, const snn_synparams *sp, int reduce, snn_stream_t stream) {
    if (!reduce_valid(reduce)) return SNN_ERR_INVALID;
    if (!W || !s_src || !x_src || !s_tgt || !x_tgt || B <= 0 || Nin <= 0 || N <= 0 || !syn_valid(sp, N)) return SNN_ERR_INVALID;
    if (sp && ((sp->nu0 && sp->nu0_rs != 0) || (sp->nu1 && sp->nu1_rs != 0))) return SNN_ERR_INVALID;     // learning.py:401-402
    if (B > 256) return SNN_ERR_UNSUPPORTED;
    StdpArgs a{.W = W, .s_src = s_src, .x_src = x_src, .s_tgt = s_tgt, .x_tgt = x_tgt, .B = B, .Nin = Nin, .N = N, .nu0 = nu0, .nu1 = nu1,
               .use_dt = use_dt, .dt = dt, .decay = decay, .has_min = has_min, .wmin = wmin, .has_max = has_max, .wmax = wmax,
               .assume_clamped = (assume_clamped && decay == 1.0f) ? 1 : 0, .mode = 0, .reward = 0.f, .reward_vec = nullptr};
    if (sp) syn_rates(a, *sp);                           // (a tensor rate makes the instance per-synapse: nothing changes on the scalar path)
    return launch_plasticity_for(a, sp, reduce, (hipStream_t)stream);
}

extern "C" int snn_stdp_postpre_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                                    int Nin, int N, float nu0, float nu1, int use_dt, float dt, float decay, int has_min, float wmin,
                                    int has_max, float wmax, int assume_clamped, const snn_synparams *sp, int reduce, snn_stream_t stream) {
    return postpre_dense(W, s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, use_dt, dt, decay, has_min, wmin, has_max, wmax, assume_clamped,
                         sp, reduce, stream);
}

extern "C" int snn_stdp_postpre_pv(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                                   int Nin, int N, float nu0, float nu1, int use_dt, float dt, float decay, int has_min, float wmin,
                                   int has_max, float wmax, int assume_clamped, const snn_synparams *sp, snn_stream_t stream) {
    return postpre_dense(W, s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, use_dt, dt, decay, has_min, wmin, has_max, wmax, assume_clamped,
                         sp, SNN_REDUCE_SUM, stream);
}

extern "C" int snn_stdp_postpre(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                                const float *x_tgt, int B, int Nin, int N, float nu0, float nu1, int use_dt,
                                float dt, float decay, int has_min, float wmin, int has_max, float wmax,
                                int assume_clamped, snn_stream_t stream) {
    return postpre_dense(W, s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, use_dt, dt, decay, has_min, wmin, has_max, wmax, assume_clamped,
                         nullptr, SNN_REDUCE_SUM, stream);
}

__global__ __launch_bounds__(256) void k_mstdp_traces(float *__restrict__ p_plus, float *__restrict__ p_minus,
                                                      uint8_t *__restrict__ s_src_prev,
                                                      uint8_t *__restrict__ s_tgt_prev,
                                                      const uint8_t *__restrict__ s_src,
                                                      const uint8_t *__restrict__ s_tgt, long n_src, long n_tgt,
                                                      float a_plus, float a_minus, float d_plus, float d_minus) {
    const long n = n_src + n_tgt;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x) {
        if (k < n_src) {
            const uint8_t sv = s_src[k];
            const float p = p_plus[k] * d_plus;                  // learning.py:1564
            p_plus[k] = p + a_plus * (float)sv;                  // :1565
            s_src_prev[k] = sv;
        } else {
            const long q = k - n_src;
            const uint8_t sv = s_tgt[q];
            const float p = p_minus[q] * d_minus;                // :1566
            p_minus[q] = p + a_minus * (float)sv;                // :1567
            s_tgt_prev[q] = sv;
        }
    }
}

// The traces behind an MSTDP / MSTDPET update: p_plus / p_minus decay and take this step's spikes, which are remembered as the factors of
// the next eligibility.  `max_blocks` > 0 caps the grid (MSTDP's B * (Nin + N) elements); 0: one thread per element (MSTDPET, batch 1).
static int launch_mstdp_traces(float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                               const uint8_t *s_tgt, long n_src, long n_tgt, float a_plus, float a_minus, float decay_plus, float decay_minus,
                               long max_blocks, hipStream_t st) {
    long blocks = (n_src + n_tgt + 255) / 256;
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    hipLaunchKernelGGL(k_mstdp_traces, dim3((unsigned)blocks), dim3(256), 0, st, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, n_src,
                       n_tgt, a_plus, a_minus, decay_plus, decay_minus);
    return snn_check_launch();
}

// f4: PostPre on a Conv2dConnection (learning.py:457-497).  Phase 1: one thread per (sample, weight element) sums its
// products over the output positions l in ascending order; phase 2: one thread per weight element reduces the samples in
// ATen's sum(dim=0) order, applies the learning rates, decay and clamp.
__global__ __launch_bounds__(256) void k_conv_pp_partial(const uint8_t *__restrict__ s_src, const float *__restrict__ x_src,
                                                         const uint8_t *__restrict__ s_tgt, const float *__restrict__ x_tgt,
                                                         float *__restrict__ part, int B, int Cin, int H, int Wd, int Cout, int KH,
                                                         int KW, int stride, int pad, int OH, int OW) {
    const long K = (long)Cin * KH * KW, E = (long)Cout * K;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long)B * E) return;
    const int b = (int)(id / E);
    const long e = id - (long)b * E;
    const int co = (int)(e / K), k = (int)(e - (long)co * K);
    const int ci = k / (KH * KW), ky = (k / KW) % KH, kx = k % KW;
    const int L = OH * OW;
    float a = 0.f, p = 0.f;
    for (int l = 0; l < L; ++l) {
        const int oy = l / OW, ox = l - oy * OW;
        const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
        const bool in = iy >= 0 && iy < H && ix >= 0 && ix < Wd;
        const size_t si = (((size_t)b * Cin + ci) * H + (in ? iy : 0)) * Wd + (in ? ix : 0);
        const size_t ti = ((size_t)b * Cout + co) * L + l;
        a += x_tgt[ti] * (in ? (float)s_src[si] : 0.0f);
        p += (float)s_tgt[ti] * (in ? x_src[si] : 0.0f);
    }
    part[id] = a;
    part[(size_t)B * E + id] = p;
}

// The same partial sums from packed spike rows (snn_conv_events.hpp): a workgroup = one (sample, input channel, slice of 256
// weight elements); it packs the sample's source rows of that channel and ALL its target rows into LDS words (one per image
// row), then every thread walks the set bits its element reads.  Bit-identical to k_conv_pp_partial (checked body against body
// on the host: tests/test_conv_events_host.py); rows wider than 32 pixels never get here, multi-valued spike bytes take the
// dense body.  The default since round 4 (first run on an MI355X: parity tests green, 8 879 vs 4 361 timesteps/s on the
// Conv2d 5x5x32 PostPre graph at B = 16, profiles/r04_conv_postpre_dense_vs_events.jsonl); SNN_CONV_PP_EVENTS=0 selects the dense body.
__global__ __launch_bounds__(256) void k_conv_pp_partial_ev(const uint8_t *__restrict__ s_src, const float *__restrict__ x_src,
                                                            const uint8_t *__restrict__ s_tgt, const float *__restrict__ x_tgt,
                                                            float *__restrict__ part, int B, snn::ConvGeom g) {
    // Round 6: a workgroup = (sample, input channel, chunk of CO output channels) and stages what its elements read -- the chunk's target
    // traces, the channel's source traces, the packed spike rows -- in LDS: the walk over the events used to chase one global load per
    // event (40 us per call at the conv_mnist.py shapes; every workgroup also packed ALL target rows of its sample).
    constexpr int CO = 8;
    extern __shared__ uint32_t ev_lds[];                 // srow[H] | trow[CO * OH] | multi | xt[CO * OH * OW] | xs[H * Wd]
    const int L = g.OH * g.OW;
    uint32_t *srow = ev_lds, *trow = ev_lds + g.H;
    int *multi = (int *)(trow + CO * g.OH);
    float *xt = (float *)(multi + 1), *xs = xt + CO * L;
    const int tid = threadIdx.x, b = blockIdx.x / g.Cin, ci = blockIdx.x - b * g.Cin;
    const int co0 = blockIdx.y * CO, nco = min(CO, g.Cout - co0);
    if (tid == 0) *multi = 0;
    __syncthreads();
    const size_t soff = ((size_t)b * g.Cin + ci) * g.H * g.Wd, toff0 = ((size_t)b * g.Cout + co0) * L;
    int mine = 0;
    // (conv_pack_row's result from 4-byte loads where the row starts on a 4-byte boundary: a row of 24 / 28 bytes is 6 / 7 loads, not 24 / 28)
    auto pack = [&](const uint8_t *row, int n) -> uint32_t {
        if ((((uintptr_t)row) & 3) != 0) return snn::conv_pack_row(row, n, &mine);
        uint32_t m = 0;
        int x = 0;
        for (; x + 4 <= n; x += 4) {
            const uint32_t v = *(const uint32_t *)(row + x);
            if (v & 0xFEFEFEFEu) mine = 1;
            const uint32_t nz = (v | ((v & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;      // byte k non-zero -> bit 8k+7
            m |= (((nz >> 7) | (nz >> 14) | (nz >> 21) | (nz >> 28)) & 0xFu) << x;
        }
        for (; x < n; ++x) { const uint8_t v = row[x]; m |= (uint32_t)(v != 0) << x; if (v > 1) mine = 1; }
        return m;
    };
    for (int r = tid; r < g.H; r += 256) srow[r] = pack(s_src + soff + (size_t)r * g.Wd, g.Wd);
    for (int r = tid; r < nco * g.OH; r += 256) trow[r] = pack(s_tgt + toff0 + (size_t)r * g.OW, g.OW);
    for (int k = tid; k < nco * L; k += 256) xt[k] = x_tgt[toff0 + k];
    for (int k = tid; k < g.H * g.Wd; k += 256) xs[k] = x_src[soff + k];
    if (mine) atomicOr(multi, 1);
    __syncthreads();
    const bool dense = *multi != 0;
    const int KK = g.KH * g.KW;
    const long K = (long)g.Cin * KK, E = (long)g.Cout * K;
    if (tid >= nco * KK) return;
    const int cl = tid / KK, kk = tid - cl * KK, ky = kk / g.KW, kx = kk - ky * g.KW, co = co0 + cl;
    float a, p;
    if (!dense) snn::conv_pp_events(g, ky, kx, srow, trow + cl * g.OH, xs, xt + cl * L, &a, &p);
    else snn::conv_pp_dense(g, ky, kx, s_src + soff, xs, s_tgt + toff0 + (size_t)cl * L, xt + cl * L, &a, &p);
    const long id = (long)b * E + (long)co * K + (long)ci * KK + kk;
    part[id] = a;
    part[(size_t)B * E + id] = p;
}

// phase 2: one thread per weight element reduces the samples' partial sums (conv_pp_batch_sum, snn_conv_apply.hpp) and applies rates, decay and clamp
template <class ACC = OuterSum>
__global__ __launch_bounds__(256) void k_conv_pp_apply(float *__restrict__ W, const float *__restrict__ part, int B, long E, float nu0,
                                                       float nu1, float decay, int has_min, float wmin, int has_max, float wmax) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const bool tail = e >= (E / 32) * 32;
    float w = W[e];
    if (nu0 != 0.f) w = w - nu0 * conv_pp_batch_sum<ACC>(part, B, E, e, tail);
    if (nu1 != 0.f) w = w + nu1 * conv_pp_batch_sum<ACC>(part + (size_t)B * E, B, E, e, tail);
    w = w * decay;
    if (has_min && w < wmin) w = wmin;
    if (has_max && w > wmax) w = wmax;
    W[e] = w;
}

// phase 1 of the conv2d outer-product rules (PostPre, Hebbian, WeightDependentPostPre): ws <- [pre | post][B][E] per-sample partial sums
static int conv_pp_partials(const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Cin, int H, int Wd,
                            int Cout, int KH, int KW, int stride, int pad, int OH, int OW, float *ws, hipStream_t stream) {
    const long E = (long)Cout * Cin * KH * KW, n = (long)B * E;
    static const bool events = [] { const char *v = getenv("SNN_CONV_PP_EVENTS"); return !(v && v[0] == '0'); }();
    const size_t ev_lds_bytes = ((size_t)H + (size_t)8 * OH + 1) * sizeof(uint32_t) + ((size_t)8 * OH * OW + (size_t)H * Wd) * sizeof(float);
    if (events && Wd <= 32 && OW <= 32 && ev_lds_bytes <= 60 * 1024 && 8 * KH * KW <= 256) {
        const snn::ConvGeom g{Cin, H, Wd, Cout, KH, KW, stride, pad, OH, OW};
        hipLaunchKernelGGL(k_conv_pp_partial_ev, dim3((unsigned)(B * Cin), (unsigned)((Cout + 7) / 8)), dim3(256), ev_lds_bytes,
                           (hipStream_t)stream, s_src, x_src, s_tgt, x_tgt, ws, B, g);
    } else {
        hipLaunchKernelGGL(k_conv_pp_partial, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s_src, x_src, s_tgt, x_tgt, ws,
                           B, Cin, H, Wd, Cout, KH, KW, stride, pad, OH, OW);
    }
    return SNN_OK;
}

extern "C" int snn_conv2d_postpre_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                                      int B, int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad, float nu0, float nu1,
                                      float decay, int has_min, float wmin, int has_max, float wmax, float *ws, int reduce,
                                      snn_stream_t stream) {
    if (!reduce_valid(reduce)) return SNN_ERR_INVALID;
    if (!W || !s_src || !x_src || !s_tgt || !x_tgt || !ws || B <= 0 || Cin <= 0 || H <= 0 || Wd <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 ||
        stride <= 0 || pad < 0) return SNN_ERR_INVALID;
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (Wd + 2 * pad - KW) / stride + 1;
    if (OH <= 0 || OW <= 0) return SNN_ERR_INVALID;
    const long E = (long)Cout * Cin * KH * KW;
    const int rc = conv_pp_partials(s_src, x_src, s_tgt, x_tgt, B, Cin, H, Wd, Cout, KH, KW, stride, pad, OH, OW, ws, (hipStream_t)stream);
    if (rc) return rc;
    const dim3 grid((unsigned)((E + 255) / 256));
    auto apply = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, W, (const float *)ws, B, E, nu0, nu1, decay, has_min, wmin, has_max, wmax);
    };
    if (reduce == SNN_REDUCE_MEAN) apply(k_conv_pp_apply<BatchReduce<SNN_REDUCE_MEAN>>);
    else if (reduce == SNN_REDUCE_AMAX) apply(k_conv_pp_apply<BatchReduce<SNN_REDUCE_AMAX>>);
    else if (reduce == SNN_REDUCE_AMIN) apply(k_conv_pp_apply<BatchReduce<SNN_REDUCE_AMIN>>);
    else apply(k_conv_pp_apply<>);
    return snn_check_launch();
}

extern "C" int snn_conv2d_postpre(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                                  int B, int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad, float nu0, float nu1,
                                  float decay, int has_min, float wmin, int has_max, float wmax, float *ws, snn_stream_t stream) {
    return snn_conv2d_postpre_red(W, s_src, x_src, s_tgt, x_tgt, B, Cin, H, Wd, Cout, KH, KW, stride, pad, nu0, nu1, decay, has_min, wmin,
                                  has_max, wmax, ws, SNN_REDUCE_SUM, stream);
}

// Hebbian (learning.py:1348-1380) / WeightDependentPostPre (:920-976) on a Conv2dConnection: the two sums PostPre reduces (the same partial
// kernels, k_conv_pp_apply's ordered batch reduction), then the statements k_plasticity runs for the dense family (modes 2 / 3) -- except
// that the reference's `w += update` also runs when both rates are zero (update is then the integer 0: a -0.0 weight becomes +0.0).
template <class ACC = OuterSum>
__global__ __launch_bounds__(256) void k_conv_hebb_apply(float *__restrict__ W, const float *__restrict__ part, int B, long E, float nu0,
                                                         float nu1, int weight_dependent, float decay, int has_min, float wmin, int has_max,
                                                         float wmax) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const bool tail = e >= (E / 32) * 32;
    float w = W[e];
    // (Hebbian's two statements always run; WeightDependentPostPre skips a side whose rate is zero, and its loads with it)
    const float pre = (!weight_dependent || nu0 != 0.f) ? conv_pp_batch_sum<ACC>(part, B, E, e, tail) : 0.f;
    const float post = (!weight_dependent || nu1 != 0.f) ? conv_pp_batch_sum<ACC>(part + (size_t)B * E, B, E, e, tail) : 0.f;
    if (!weight_dependent) {                            // w += nu0 * pre; w += nu1 * post
        w = w + nu0 * pre;
        w = w + nu1 * post;
    } else {                                            // update = 0 - (nu0 pre)(w - wmin) + (nu1 post)(wmax - w); w += update
        float upd = 0.f;
        if (nu0 != 0.f) upd = upd - (nu0 * pre) * (w - wmin);
        if (nu1 != 0.f) upd = upd + (nu1 * post) * (wmax - w);
        w = w + upd;
    }
    w = w * decay;
    if (has_min && w < wmin) w = wmin;
    if (has_max && w > wmax) w = wmax;
    W[e] = w;
}

extern "C" int snn_conv2d_hebbian_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                                      int B, int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad, float nu0, float nu1,
                                      int weight_dependent, float decay, int has_min, float wmin, int has_max, float wmax, float *ws,
                                      int reduce, snn_stream_t stream) {
    if (!reduce_valid(reduce)) return SNN_ERR_INVALID;
    if (!W || !s_src || !x_src || !s_tgt || !x_tgt || !ws || B <= 0 || Cin <= 0 || H <= 0 || Wd <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 ||
        stride <= 0 || pad < 0) return SNN_ERR_INVALID;
    if (weight_dependent && !(has_min && has_max)) return SNN_ERR_INVALID;      // learning.py:600-602: finite wmin and wmax
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (Wd + 2 * pad - KW) / stride + 1;
    if (OH <= 0 || OW <= 0) return SNN_ERR_INVALID;
    const long E = (long)Cout * Cin * KH * KW;
    const int rc = conv_pp_partials(s_src, x_src, s_tgt, x_tgt, B, Cin, H, Wd, Cout, KH, KW, stride, pad, OH, OW, ws, (hipStream_t)stream);
    if (rc) return rc;
    const dim3 grid((unsigned)((E + 255) / 256));
    auto apply = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, W, (const float *)ws, B, E, nu0, nu1, weight_dependent, decay, has_min, wmin,
                           has_max, wmax);
    };
    if (reduce == SNN_REDUCE_MEAN) apply(k_conv_hebb_apply<BatchReduce<SNN_REDUCE_MEAN>>);
    else if (reduce == SNN_REDUCE_AMAX) apply(k_conv_hebb_apply<BatchReduce<SNN_REDUCE_AMAX>>);
    else if (reduce == SNN_REDUCE_AMIN) apply(k_conv_hebb_apply<BatchReduce<SNN_REDUCE_AMIN>>);
    else apply(k_conv_hebb_apply<>);
    return snn_check_launch();
}

extern "C" int snn_conv2d_hebbian(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                                  int B, int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad, float nu0, float nu1,
                                  int weight_dependent, float decay, int has_min, float wmin, int has_max, float wmax, float *ws,
                                  snn_stream_t stream) {
    return snn_conv2d_hebbian_red(W, s_src, x_src, s_tgt, x_tgt, B, Cin, H, Wd, Cout, KH, KW, stride, pad, nu0, nu1, weight_dependent, decay,
                                  has_min, wmin, has_max, wmax, ws, SNN_REDUCE_SUM, stream);
}

// MSTDP on a Conv2dConnection (learning.py:1942-2015, batch 1).  State: E = eligibility [Cout, K], P = P^+ in input space
// [Cin, H, W] (the reference's unfolded copy goes through the same elementwise operations), Q = P^- [Cout, L].
// (1) w += nu0 * sum_over_output_channels(reward * E) -- the reference's torch.sum(update, dim=0) on a weight-shaped
//     eligibility, broadcast back over the channels --, decay, clamp; one thread per kernel tap k, ATen order over co.
__global__ __launch_bounds__(256) void k_conv_mstdp_apply(float *__restrict__ W, const float *__restrict__ E, int Cout, long K, float reward,
                                                          float nu0, float wdecay, int has_min, float wmin, int has_max, float wmax) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    OuterSum acc; acc.init(k >= (K / 32) * 32);
    for (int co = 0; co < Cout; ++co) acc.add(co, reward * E[(long)co * K + k], Cout);
    const float S = acc.finish(Cout);
    for (int co = 0; co < Cout; ++co) {
        float w = W[(long)co * K + k] + nu0 * S;
        w = w * wdecay;
        if (has_min && w < wmin) w = wmin;
        if (has_max && w > wmax) w = wmax;
        W[(long)co * K + k] = w;
    }
}

// (2) P = P * decay_plus + a_plus * s_src;  Q = Q * decay_minus + a_minus * s_tgt   (learning.py:1998-2001)
__global__ __launch_bounds__(256) void k_conv_mstdp_traces(float *__restrict__ P, float *__restrict__ Q, const uint8_t *__restrict__ s_src,
                                                           const uint8_t *__restrict__ s_tgt, long nP, long nQ, float a_plus,
                                                           float a_minus, float decay_plus, float decay_minus) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < nP) { const float p = P[i] * decay_plus; P[i] = p + a_plus * (float)s_src[i]; }
    else if (i < nP + nQ) { const long q = i - nP; const float v = Q[q] * decay_minus; Q[q] = v + a_minus * (float)s_tgt[q]; }
}

// (3) E[co,k] = sum_l s_tgt[co,l] * unfold(P)[k,l] + sum_l Q[co,l] * unfold(s_src)[k,l], each sum ascending in l (the
//     canonical order pinned for the reference's two torch.bmm calls, :2004-2007)
__global__ __launch_bounds__(256) void k_conv_mstdp_elig(float *__restrict__ E, const float *__restrict__ P, const float *__restrict__ Q,
                                                         const uint8_t *__restrict__ s_src, const uint8_t *__restrict__ s_tgt, int Cin,
                                                         int H, int Wd, int Cout, int KH, int KW, int stride, int pad, int OH, int OW) {
    const long K = (long)Cin * KH * KW;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)Cout * K) return;
    const int co = (int)(e / K), k = (int)(e - (long)co * K);
    const int ci = k / (KH * KW), ky = (k / KW) % KH, kx = k % KW;
    const int L = OH * OW;
    float a = 0.f, b = 0.f;
    for (int l = 0; l < L; ++l) {
        const int oy = l / OW, ox = l - oy * OW;
        const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
        const bool in = iy >= 0 && iy < H && ix >= 0 && ix < Wd;
        const size_t si = ((size_t)ci * H + (in ? iy : 0)) * Wd + (in ? ix : 0);
        a += (float)s_tgt[(size_t)co * L + l] * (in ? P[si] : 0.0f);
        b += Q[(size_t)co * L + l] * (in ? (float)s_src[si] : 0.0f);
    }
    E[e] = a + b;
}

extern "C" int snn_conv2d_mstdp_step(float *W, float *elig, float *p_plus, float *p_minus, const uint8_t *s_src, const uint8_t *s_tgt,
                                     int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad, float reward, float nu0,
                                     float a_plus, float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min,
                                     float wmin, int has_max, float wmax, snn_stream_t stream) {
    if (!W || !elig || !p_plus || !p_minus || !s_src || !s_tgt || Cin <= 0 || H <= 0 || Wd <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 ||
        stride <= 0 || pad < 0) return SNN_ERR_INVALID;
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (Wd + 2 * pad - KW) / stride + 1;
    if (OH <= 0 || OW <= 0) return SNN_ERR_INVALID;
    const long K = (long)Cin * KH * KW, nP = (long)Cin * H * Wd, nQ = (long)Cout * OH * OW;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_conv_mstdp_apply, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, W, elig, Cout, K, reward, nu0, wdecay,
                       has_min, wmin, has_max, wmax);
    hipLaunchKernelGGL(k_conv_mstdp_traces, dim3((unsigned)((nP + nQ + 255) / 256)), dim3(256), 0, st, p_plus, p_minus, s_src, s_tgt, nP, nQ,
                       a_plus, a_minus, decay_plus, decay_minus);
    hipLaunchKernelGGL(k_conv_mstdp_elig, dim3((unsigned)((Cout * K + 255) / 256)), dim3(256), 0, st, elig, p_plus, p_minus, s_src, s_tgt,
                       Cin, H, Wd, Cout, KH, KW, stride, pad, OH, OW);
    return snn_check_launch();
}

// f3: Hebbian (weight_dependent = 0) / WeightDependentPostPre (1).  A bound of the weight-dependent form may come from `sp`.
static int hebbian_dense(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Nin, int N,
                         float nu0, float nu1, int weight_dependent, float decay, int has_min, float wmin, int has_max, float wmax,
                         const snn_synparams *sp, int reduce, snn_stream_t stream) {
    if (!reduce_valid(reduce)) return SNN_ERR_INVALID;
    if (!W || !s_src || !x_src || !s_tgt || !x_tgt || B <= 0 || Nin <= 0 || N <= 0 || !syn_valid(sp, N)) return SNN_ERR_INVALID;
    if (weight_dependent && !((has_min || (sp && sp->wmin)) && (has_max || (sp && sp->wmax)))) return SNN_ERR_INVALID;   // learning.py:600-602: finite wmin and wmax
    if (B > 256) return SNN_ERR_UNSUPPORTED;
    StdpArgs a{.W = W, .s_src = s_src, .x_src = x_src, .s_tgt = s_tgt, .x_tgt = x_tgt, .B = B, .Nin = Nin, .N = N, .nu0 = nu0, .nu1 = nu1,
               .use_dt = 0, .dt = 1.f, .decay = decay, .has_min = has_min, .wmin = wmin, .has_max = has_max, .wmax = wmax,
               .assume_clamped = 0, .mode = weight_dependent ? 3 : 2, .reward = 0.f, .reward_vec = nullptr};
    if (sp) syn_rates(a, *sp);
    return launch_plasticity_for(a, sp, reduce, (hipStream_t)stream);
}

extern "C" int snn_stdp_hebbian(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                                int B, int Nin, int N, float nu0, float nu1, int weight_dependent, float decay, int has_min,
                                float wmin, int has_max, float wmax, snn_stream_t stream) {
    return hebbian_dense(W, s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, weight_dependent, decay, has_min, wmin, has_max, wmax, nullptr,
                         SNN_REDUCE_SUM, stream);
}

extern "C" int snn_stdp_hebbian_pv(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                                   int Nin, int N, float nu0, float nu1, int weight_dependent, float decay, int has_min, float wmin,
                                   int has_max, float wmax, const snn_synparams *sp, snn_stream_t stream) {
    return hebbian_dense(W, s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, weight_dependent, decay, has_min, wmin, has_max, wmax, sp,
                         SNN_REDUCE_SUM, stream);
}

extern "C" int snn_stdp_hebbian_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                                    int Nin, int N, float nu0, float nu1, int weight_dependent, float decay, int has_min, float wmin,
                                    int has_max, float wmax, const snn_synparams *sp, int reduce, snn_stream_t stream) {
    return hebbian_dense(W, s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, weight_dependent, decay, has_min, wmin, has_max, wmax, sp,
                         reduce, stream);
}

// The per-synapse instance of k_mstdpet: the element's own nu0 inside ((nu0 * dt) * reward), its own bounds in the clamp.
__global__ __launch_bounds__(256) void k_mstdpet_pv(float *__restrict__ W, float *__restrict__ e_trace, const float *__restrict__ p_plus,
                                                    const float *__restrict__ p_minus, const uint8_t *__restrict__ s_src_prev,
                                                    const uint8_t *__restrict__ s_tgt_prev, int Nin, int N, float nu0, float dt, float reward,
                                                    float decay_e, float tc_e, float wdecay, int has_min, float wmin, int has_max,
                                                    float wmax, snn_synparams q) {
    const long E = (long)Nin * N;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long)gridDim.x * blockDim.x) {
        const int i = (int)(e / N), j = (int)(e - (long)i * N);
        const SynElem c = syn_elem(q, nu0, 0.f, has_min, wmin, has_max, wmax, i, j);
        const float el = p_plus[i] * (float)s_tgt_prev[j] + (float)s_src_prev[i] * p_minus[j];    // :2241-2243
        const float w = syn_mstdpet(W[e], &e_trace[e], el, decay_e, tc_e, c.nu0, dt, reward);
        W[e] = syn_finish(w, wdecay, c.lo, c.hi);
    }
}

// MSTDPET (learning.py:2187-2248, batch 1): the eligibility TRACE is genuinely dense state; the point eligibility is the
// rank-2 expression of the previous step's factors and is formed on the fly.
__global__ __launch_bounds__(256) void k_mstdpet(float *__restrict__ W, float *__restrict__ e_trace, const float *__restrict__ p_plus,
                                                 const float *__restrict__ p_minus, const uint8_t *__restrict__ s_src_prev,
                                                 const uint8_t *__restrict__ s_tgt_prev, int Nin, int N, float scale, float decay_e,
                                                 float tc_e, float wdecay, int has_min, float wmin, int has_max, float wmax) {
    const long E = (long)Nin * N;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long)gridDim.x * blockDim.x) {
        const int i = (int)(e / N), j = (int)(e - (long)i * N);
        const float el = p_plus[i] * (float)s_tgt_prev[j] + (float)s_src_prev[i] * p_minus[j];    // :2241-2243
        float et = e_trace[e] * decay_e;                // :2223
        et = et + el / tc_e;                            // :2224
        e_trace[e] = et;
        float w = W[e] + scale * et;                    // :2226-2230
        w = w * wdecay;
        if (has_min && w < wmin) w = wmin;
        if (has_max && w > wmax) w = wmax;
        W[e] = w;
    }
}

// (1) the weights from the OLD p_plus / p_minus and previous-step spikes, (2) the traces.  Per-synapse nu0 / bounds: k_mstdpet_pv.
static int mstdpet_dense(float *W, float *e_trace, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev,
                         const uint8_t *s_src, const uint8_t *s_tgt, int Nin, int N, float reward, float nu0, float dt, float a_plus,
                         float a_minus, float decay_plus, float decay_minus, float decay_e, float tc_e, float wdecay, int has_min, float wmin,
                         int has_max, float wmax, const snn_synparams *sp, snn_stream_t stream) {
    if (!W || !e_trace || !p_plus || !p_minus || !s_src_prev || !s_tgt_prev || !s_src || !s_tgt || Nin <= 0 || N <= 0 || !syn_valid(sp, N))
        return SNN_ERR_INVALID;
    const long E = (long)Nin * N;
    const unsigned grid = (unsigned)((E + 255) / 256 < 4096 ? (E + 255) / 256 : 4096);
    if (syn_any(sp)) {
        hipLaunchKernelGGL(k_mstdpet_pv, dim3(grid), dim3(256), 0, (hipStream_t)stream, W, e_trace, p_plus, p_minus, s_src_prev, s_tgt_prev,
                           Nin, N, nu0, dt, reward, decay_e, tc_e, wdecay, has_min, wmin, has_max, wmax, *sp);
    } else {
        const float scale = (nu0 * dt) * reward;        // ((nu[0] * dt) * reward) * eligibility_trace
        hipLaunchKernelGGL(k_mstdpet, dim3(grid), dim3(256), 0, (hipStream_t)stream, W, e_trace, p_plus, p_minus, s_src_prev, s_tgt_prev,
                           Nin, N, scale, decay_e, tc_e, wdecay, has_min, wmin, has_max, wmax);
    }
    int rc = snn_check_launch();
    if (rc) return rc;
    return launch_mstdp_traces(p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, Nin, N, a_plus, a_minus, decay_plus, decay_minus, 0,
                               (hipStream_t)stream);
}

extern "C" int snn_mstdpet_step(float *W, float *e_trace, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev,
                                const uint8_t *s_src, const uint8_t *s_tgt, int Nin, int N, float reward, float nu0, float dt,
                                float a_plus, float a_minus, float decay_plus, float decay_minus, float decay_e, float tc_e,
                                float wdecay, int has_min, float wmin, int has_max, float wmax, snn_stream_t stream) {
    return mstdpet_dense(W, e_trace, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, Nin, N, reward, nu0, dt, a_plus, a_minus,
                         decay_plus, decay_minus, decay_e, tc_e, wdecay, has_min, wmin, has_max, wmax, nullptr, stream);
}

extern "C" int snn_mstdpet_step_pv(float *W, float *e_trace, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev,
                                   const uint8_t *s_src, const uint8_t *s_tgt, int Nin, int N, float reward, float nu0, float dt,
                                   float a_plus, float a_minus, float decay_plus, float decay_minus, float decay_e, float tc_e,
                                   float wdecay, int has_min, float wmin, int has_max, float wmax, const snn_synparams *sp,
                                   snn_stream_t stream) {
    return mstdpet_dense(W, e_trace, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, Nin, N, reward, nu0, dt, a_plus, a_minus,
                         decay_plus, decay_minus, decay_e, tc_e, wdecay, has_min, wmin, has_max, wmax, sp, stream);
}

// MSTDP (StdpArgs mode 1).  (1) W += nu0 * reduce_b reward * elig_prev[b]; decay; clamp -- uses the OLD p_plus / p_minus; with another
// reduction the samples without a previous-step spike on the element are zero terms.  (2) the traces.
static int mstdp_dense(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                       const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0, float a_plus,
                       float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin, int has_max, float wmax,
                       const snn_synparams *sp, int reduce, snn_stream_t stream) {
    if (!reduce_valid(reduce)) return SNN_ERR_INVALID;
    if (!W || !p_plus || !p_minus || !s_src_prev || !s_tgt_prev || !s_src || !s_tgt || B <= 0 || Nin <= 0 || N <= 0 || !syn_valid(sp, N))
        return SNN_ERR_INVALID;
    if (B > 256) return SNN_ERR_UNSUPPORTED;
    const StdpArgs a{.W = W, .s_src = s_src_prev, .x_src = p_plus, .s_tgt = s_tgt_prev, .x_tgt = p_minus, .B = B, .Nin = Nin, .N = N,
                     .nu0 = nu0, .nu1 = 0.f, .use_dt = 0, .dt = 1.f, .decay = wdecay, .has_min = has_min, .wmin = wmin, .has_max = has_max,
                     .wmax = wmax, .assume_clamped = 0, .mode = 1, .reward = reward, .reward_vec = reward_vec};
    int rc = launch_plasticity_for(a, sp, reduce, (hipStream_t)stream);      // (nu0 is read per element through syn_elem: no syn_rates)
    if (rc) return rc;
    return launch_mstdp_traces(p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, (long)B * Nin, (long)B * N, a_plus, a_minus, decay_plus,
                               decay_minus, 2048, (hipStream_t)stream);
}

extern "C" int snn_mstdp_step(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev,
                              const uint8_t *s_src, const uint8_t *s_tgt, int B, int Nin, int N, float reward,
                              const float *reward_vec, float nu0, float a_plus, float a_minus, float decay_plus,
                              float decay_minus, float wdecay, int has_min, float wmin, int has_max, float wmax,
                              snn_stream_t stream) {
    return mstdp_dense(W, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, B, Nin, N, reward, reward_vec, nu0, a_plus, a_minus,
                       decay_plus, decay_minus, wdecay, has_min, wmin, has_max, wmax, nullptr, SNN_REDUCE_SUM, stream);
}

extern "C" int snn_mstdp_step_pv(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                                 const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0,
                                 float a_plus, float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin,
                                 int has_max, float wmax, const snn_synparams *sp, snn_stream_t stream) {
    return mstdp_dense(W, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, B, Nin, N, reward, reward_vec, nu0, a_plus, a_minus,
                       decay_plus, decay_minus, wdecay, has_min, wmin, has_max, wmax, sp, SNN_REDUCE_SUM, stream);
}

extern "C" int snn_mstdp_step_red(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                                  const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0,
                                  float a_plus, float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin,
                                  int has_max, float wmax, const snn_synparams *sp, int reduce, snn_stream_t stream) {
    return mstdp_dense(W, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, B, Nin, N, reward, reward_vec, nu0, a_plus, a_minus,
                       decay_plus, decay_minus, wdecay, has_min, wmin, has_max, wmax, sp, reduce, stream);
}

// =============================================================================================
// a11: normalize.  k_colsum: column sums in ATen's sum(dim=0) order; k_scale: elementwise W *= norm * (1/colsum).
// =============================================================================================
// The ATen order leaves a lot of parallelism without changing a single rounding:
//  * multi_row_sum columns (j < 32*floor(N/32)): the sums of the 16-row blocks are independent of each other (each a
//    plain sequential sum of its 16 terms); only folding them through the upper cascade levels is sequential.
//  * row_sum columns: four interleaved lanes (row mod 4), each lane again a cascade over 16-position blocks.
// Workgroup = 16 consecutive columns (never straddling the class boundary, 16 | 32) x 64 block-threads: every
// thread sums one block per round (coalesced 64-byte row segments), one thread per column (or per lane) folds the
// round's block sums in block order.
constexpr int kCsCols = 16, kCsBlk = 64;
// NV: the per-target form (snn_normalize_pv): scale[j] = norm_vec[j] / colsum, one division (syn_norm_scale).
template <bool NV>
__device__ __forceinline__ void colsum_body(const float *__restrict__ W, int Nin, int N, float norm, const float *__restrict__ norm_vec,
                                            int use_abs, float *__restrict__ scale) {
    __shared__ float bs[kCsBlk][kCsCols + 1];          // block sums of one round: [block thread][column]
    __shared__ float lanes[4][kCsCols + 1];
    const int tid = threadIdx.x, cl = tid % kCsCols, bt = tid / kCsCols;
    const int j = blockIdx.x * kCsCols + cl;
    const bool valid = j < N;
    const int jc = valid ? j : N - 1;
    const bool tail = blockIdx.x * kCsCols >= (N / 32) * 32;      // uniform per workgroup
    if (!tail) {
        const int nfull = Nin >> 4;
        float a1 = 0.f, a2 = 0.f, a3 = 0.f;            // upper cascade levels (bt == 0 threads)
        for (int base = 0; base < nfull; base += kCsBlk) {
            const int blk = base + bt;
            if (blk < nfull) {
                float v[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) { const float w = W[(size_t)(blk * 16 + k) * N + jc]; v[k] = use_abs ? fabsf(w) : w; }
                float a0 = 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k) a0 += v[k];
                bs[bt][cl] = a0;
            }
            __syncthreads();
            if (bt == 0)
                for (int b2 = base; b2 < min(nfull, base + kCsBlk); ++b2) {
                    a1 += bs[b2 - base][cl];
                    const int m = b2 + 1;              // boundary after this block
                    if ((m & 15) == 0) { a2 += a1; a1 = 0.f; if ((m & 255) == 0) { a3 += a2; a2 = 0.f; } }
                }
            __syncthreads();
        }
        if (bt == 0 && valid) {
            float a0 = 0.f;                            // rows past the last complete block
            for (int i = nfull * 16; i < Nin; ++i) { const float w = W[(size_t)i * N + jc]; a0 += use_abs ? fabsf(w) : w; }
            float cs = ((a0 + a1) + a2) + a3;
            if (NV) { scale[j] = syn_norm_scale(norm_vec[j], cs); return; }
            if (cs == 0.f) cs = 1.0f;                   // topology_features.py:265
            scale[j] = (1.0f / cs) * norm;              // torch: python_scalar / tensor == reciprocal * scalar
        }
        return;
    }
    // row_sum columns: thread = (column cl, lane s4, block group bg); lane s4 owns the rows 4p + s4, p < n4
    const int s4 = bt & 3, bg = bt >> 2;               // 16 block groups
    const int n4 = Nin >> 2, nf4 = n4 >> 4;
    float a1 = 0.f, a2 = 0.f, a3 = 0.f;                // (bg == 0 threads)
    for (int base = 0; base < nf4; base += kCsBlk / 4) {
        const int blk = base + bg;
        if (blk < nf4) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) { const float w = W[(size_t)(4 * (blk * 16 + k) + s4) * N + jc]; v[k] = use_abs ? fabsf(w) : w; }
            float a0 = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) a0 += v[k];
            bs[bt][cl] = a0;
        }
        __syncthreads();
        if (bg == 0)
            for (int b2 = base; b2 < min(nf4, base + kCsBlk / 4); ++b2) {
                a1 += bs[(b2 - base) * 4 + s4][cl];
                const int m = b2 + 1;
                if ((m & 15) == 0) { a2 += a1; a1 = 0.f; if ((m & 255) == 0) { a3 += a2; a2 = 0.f; } }
            }
        __syncthreads();
    }
    if (bg == 0) {
        float a0 = 0.f;                                // positions past the lane's last complete block
        for (int p_ = nf4 * 16; p_ < n4; ++p_) { const float w = W[(size_t)(4 * p_ + s4) * N + jc]; a0 += use_abs ? fabsf(w) : w; }
        float lane = ((a0 + a1) + a2) + a3;
        if (s4 == 0)                                   // the Nin % 4 leftover rows join lane 0 after its cascade
            for (int i = n4 * 4; i < Nin; ++i) { const float w = W[(size_t)i * N + jc]; lane += use_abs ? fabsf(w) : w; }
        lanes[s4][cl] = lane;
    }
    __syncthreads();
    if (bt == 0 && valid) {
        float cs = ((lanes[0][cl] + lanes[1][cl]) + lanes[2][cl]) + lanes[3][cl];
        if (NV) { scale[j] = syn_norm_scale(norm_vec[j], cs); return; }
        if (cs == 0.f) cs = 1.0f;
        scale[j] = (1.0f / cs) * norm;
    }
}

__global__ __launch_bounds__(kCsCols * kCsBlk) void k_colsum(const float *__restrict__ W, int Nin, int N, float norm,
                                                             int use_abs, float *__restrict__ scale) {
    colsum_body<false>(W, Nin, N, norm, nullptr, use_abs, scale);
}
__global__ __launch_bounds__(kCsCols * kCsBlk) void k_colsum_nv(const float *__restrict__ W, int Nin, int N,
                                                                const float *__restrict__ norm_vec, int use_abs,
                                                                float *__restrict__ scale) {
    colsum_body<true>(W, Nin, N, 0.f, norm_vec, use_abs, scale);
}

// Fewer than 8 columns where colsum_body's two uniform column classes do not describe ATen's order: ONE column is an inner reduction
// (inner_sum8_terms), four to seven columns put the first four on the cascade and the rest on row_sum (outer_tail).  One thread
// per column: a layer of fewer than eight neurons is no hot path.
template <bool NV>
__global__ __launch_bounds__(64) void k_colsum_few(const float *__restrict__ W, int Nin, int N, float norm, const float *__restrict__ norm_vec,
                                                   int use_abs, float *__restrict__ scale) {
    const int j = threadIdx.x;
    if (j >= N) return;
    auto term = [=](int i) { const float w = W[(size_t)i * N + j]; return use_abs ? fabsf(w) : w; };
    float cs;
    if (N == 1) {
        cs = inner_sum8_terms(term, Nin);
    } else {
        OuterSum acc; acc.init(outer_tail(j, N));
        for (int i = 0; i < Nin; ++i) acc.add(i, term(i), Nin);
        cs = acc.finish(Nin);
    }
    if (NV) { scale[j] = syn_norm_scale(norm_vec[j], cs); return; }
    if (cs == 0.f) cs = 1.0f;
    scale[j] = (1.0f / cs) * norm;
}
static bool colsum_is_few(int N) { return N == 1 || (N >= 4 && N < 8); }

__global__ __launch_bounds__(256) void k_scale_cols(float *__restrict__ W, long E, int N,
                                                    const float *__restrict__ scale) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (long)gridDim.x * blockDim.x)
        W[e] = W[e] * scale[e % N];
}

extern "C" int snn_normalize(float *W, int Nin, int N, float norm, int use_abs, float *colsum_ws,
                             snn_stream_t stream) {
    if (!W || !colsum_ws || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (Nin > kMaxTerms) return SNN_ERR_UNSUPPORTED;
    if (colsum_is_few(N))
        hipLaunchKernelGGL(k_colsum_few<false>, dim3(1), dim3(64), 0, (hipStream_t)stream, W, Nin, N, norm, (const float *)nullptr, use_abs,
                           colsum_ws);
    else
        hipLaunchKernelGGL(k_colsum, dim3((N + kCsCols - 1) / kCsCols), dim3(kCsCols * kCsBlk), 0, (hipStream_t)stream, W, Nin, N,
                           norm, use_abs, colsum_ws);
    int rc = snn_check_launch();
    if (rc) return rc;
    const long E = (long)Nin * N;
    const unsigned grid = (unsigned)((E + 255) / 256 < 4096 ? (E + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_scale_cols, dim3(grid), dim3(256), 0, (hipStream_t)stream, W, E, N, colsum_ws);
    return snn_check_launch();
}

extern "C" int snn_normalize_pv(float *W, int Nin, int N, const float *norm_vec, int use_abs, float *colsum_ws, snn_stream_t stream) {
    if (!W || !norm_vec || !colsum_ws || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (Nin > kMaxTerms) return SNN_ERR_UNSUPPORTED;
    if (colsum_is_few(N))
        hipLaunchKernelGGL(k_colsum_few<true>, dim3(1), dim3(64), 0, (hipStream_t)stream, W, Nin, N, 0.f, norm_vec, use_abs, colsum_ws);
    else
        hipLaunchKernelGGL(k_colsum_nv, dim3((N + kCsCols - 1) / kCsCols), dim3(kCsCols * kCsBlk), 0, (hipStream_t)stream, W, Nin, N,
                           norm_vec, use_abs, colsum_ws);
    int rc = snn_check_launch();
    if (rc) return rc;
    const long E = (long)Nin * N;
    const unsigned grid = (unsigned)((E + 255) / 256 < 4096 ? (E + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_scale_cols, dim3(grid), dim3(256), 0, (hipStream_t)stream, W, E, N, colsum_ws);
    return snn_check_launch();
}

// a11 for Conv2dConnection: normalize(), bindsnet/network/topology.py:824-837.  Every [KH*KW] filter of the [Cout*Cin, KH*KW] view
// is scaled to sum `norm`: w[f] *= norm / w[f].sum(0), where the sum is ATen's vectorised INNER sum (snn_order.hpp inner_sum8) and
// torch evaluates float / tensor as reciprocal(sum) * norm.  No zero guard (the reference has none).  One thread per filter: the
// weights of a convolution are a few hundred floats.  The body is __host__ __device__ and checked on the host against the reference
// fixture (tests/test_order_rng_host.py); first run on an MI355X in round 4 (reference fixture bit for bit, profiles/r04_experimental_suite_mi355x.log).
__global__ __launch_bounds__(64) void k_normalize_filters(float *__restrict__ W, int F, int K, float norm) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    float *w = W + (size_t)f * K;
    const float sum = inner_sum8(w, K);
    const float rc = 1.0f / sum;
    const float scale = rc * norm;
    for (int k = 0; k < K; ++k) w[k] = w[k] * scale;
}

extern "C" int snn_normalize_conv2d(float *W, int n_filters, int taps, float norm, snn_stream_t stream) {
    if (!W || n_filters <= 0 || taps <= 0) return SNN_ERR_INVALID;
    if (taps > kMaxTerms) return SNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_normalize_filters, dim3((unsigned)((n_filters + 63) / 64)), dim3(64), 0, (hipStream_t)stream, W, n_filters, taps, norm);
    return snn_check_launch();
}

// =============================================================================================
// Network.reset_state_variables(): every state tensor of every layer filled in ONE launch
// (bindsnet/network/network.py:467-481 -> nodes.py:109-120, 531-538, 1113-1120: s, x, refrac_count <- 0, v <- rest).
// =============================================================================================
namespace {
struct FillArgs { snn_fill_segment seg[SNN_MAX_FILL_SEGMENTS]; unsigned first_block[SNN_MAX_FILL_SEGMENTS + 1]; int n; };

__global__ __launch_bounds__(256) void k_fill_segments(const FillArgs a) {
    int k = 0;
    while (k + 1 < a.n && blockIdx.x >= a.first_block[k + 1]) ++k;          // (n <= 32: a short uniform scan)
    const snn_fill_segment sg = a.seg[k];
    const size_t off = ((size_t)(blockIdx.x - a.first_block[k]) * 256 + threadIdx.x) * 16;
    if (off >= sg.bytes) return;
    unsigned char *p = (unsigned char *)sg.ptr + off;
    if (off + 16 <= sg.bytes && (((uintptr_t)p) & 15) == 0) {
        *(uint4 *)p = make_uint4(sg.pattern, sg.pattern, sg.pattern, sg.pattern);
    } else {
        const size_t n = sg.bytes - off < 16 ? sg.bytes - off : 16;
        for (size_t b = 0; b < n; ++b) p[b] = (unsigned char)(sg.pattern >> (8 * ((off + b) & 3)));
    }
}
}  // namespace

extern "C" int snn_fill_segments(const snn_fill_segment *h_segs, int n, snn_stream_t stream) {
    if (n < 0 || (n > 0 && !h_segs)) return SNN_ERR_INVALID;
    if (n > SNN_MAX_FILL_SEGMENTS) return SNN_ERR_UNSUPPORTED;
    FillArgs a;
    a.n = 0;
    unsigned blocks = 0;
    for (int k = 0; k < n; ++k) {
        if (!h_segs[k].bytes) continue;
        if (!h_segs[k].ptr) return SNN_ERR_INVALID;
        // a non-zero pattern is a 32-bit value: the buffer must then be a whole number of aligned words
        if (h_segs[k].pattern && ((h_segs[k].bytes & 3) || (((uintptr_t)h_segs[k].ptr) & 3))) return SNN_ERR_INVALID;
        a.seg[a.n] = h_segs[k];
        a.first_block[a.n] = blocks;
        blocks += (unsigned)((h_segs[k].bytes + 4095) / 4096);
        ++a.n;
    }
    if (!a.n) return SNN_OK;
    a.first_block[a.n] = blocks;
    hipLaunchKernelGGL(k_fill_segments, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return snn_check_launch();
}

// =============================================================================================
// Monitor.record() for float state (monitors.py:94-111): timestep t's copy of every monitored tensor into its [T, ...] recording,
// ONE launch for up to SNN_MAX_RECORD_SEGMENTS tensors.  Like k_fill_segments: the table by value in the kernel arguments, a
// block-to-segment map, 4 KiB per block.  Memory-bound and tiny (a few KiB per step for the layer sizes monitors are used at):
// what counts is that it is one launch, and 16 bytes per lane where both ends allow it.
// =============================================================================================
namespace {
struct RecordSeg { const unsigned char *src; unsigned char *dst; unsigned long long bytes; };      // dst: already the slice of timestep t
struct RecordArgs { RecordSeg seg[SNN_MAX_RECORD_SEGMENTS]; unsigned first_block[SNN_MAX_RECORD_SEGMENTS + 1]; unsigned wide; int n; };

__global__ __launch_bounds__(256) void k_record_segments(const RecordArgs a) {
    int k = 0;
    while (k + 1 < a.n && blockIdx.x >= a.first_block[k + 1]) ++k;          // (n <= 32: a short uniform scan)
    const RecordSeg sg = a.seg[k];
    const size_t base = (size_t)(blockIdx.x - a.first_block[k]) * 4096;      // this block's 4 KiB of the segment
    if ((a.wide >> k) & 1u) {                                                // both ends 16-byte aligned: 16 bytes per lane, words at the tail
        const size_t off = base + (size_t)threadIdx.x * 16;
        if (off + 16 <= sg.bytes) *(uint4 *)(sg.dst + off) = *(const uint4 *)(sg.src + off);
        else for (size_t b = off; b < sg.bytes; b += 4) *(uint32_t *)(sg.dst + b) = *(const uint32_t *)(sg.src + b);
    } else {                                                                 // 4-byte aligned only: consecutive lanes, consecutive words
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t off = base + ((size_t)q * 256 + threadIdx.x) * 4;
            if (off < sg.bytes) *(uint32_t *)(sg.dst + off) = *(const uint32_t *)(sg.src + off);
        }
    }
}
}  // namespace

extern "C" int snn_record_segments(const snn_record_segment *h_segs, int n, long long t, snn_stream_t stream) {
    if (n < 0 || t < 0 || (n > 0 && !h_segs)) return SNN_ERR_INVALID;
    for (int k = 0; k < n; ++k) {              // every segment is checked before the first group is launched
        if (!h_segs[k].bytes) continue;
        if (!h_segs[k].src || !h_segs[k].dst || (h_segs[k].bytes & 3)) return SNN_ERR_INVALID;
        if ((((uintptr_t)h_segs[k].src) | ((uintptr_t)h_segs[k].dst)) & 3) return SNN_ERR_INVALID;
        if (h_segs[k].bytes > (1ull << 36)) return SNN_ERR_UNSUPPORTED;      // (32 such segments still fit the grid's 2^31 blocks)
    }
    for (int k0 = 0; k0 < n; ) {
        RecordArgs a;
        a.n = 0;
        a.wide = 0;
        unsigned blocks = 0;
        for (; k0 < n && a.n < SNN_MAX_RECORD_SEGMENTS; ++k0) {
            const snn_record_segment &h = h_segs[k0];
            if (!h.bytes) continue;
            RecordSeg &sg = a.seg[a.n];
            sg.src = (const unsigned char *)h.src;
            sg.dst = (unsigned char *)h.dst + (size_t)t * h.bytes;
            sg.bytes = h.bytes;
            if (((((uintptr_t)sg.src) | ((uintptr_t)sg.dst)) & 15) == 0) a.wide |= 1u << a.n;
            a.first_block[a.n] = blocks;
            blocks += (unsigned)((h.bytes + 4095) / 4096);
            ++a.n;
        }
        if (!a.n) continue;
        a.first_block[a.n] = blocks;
        hipLaunchKernelGGL(k_record_segments, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
        const int rc = snn_check_launch();
        if (rc) return rc;
    }
    return SNN_OK;
}
