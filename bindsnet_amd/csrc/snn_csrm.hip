// snn_csrm.hip -- CSRMNodes (bindsnet/network/nodes.py:1319-1552): the windowed propagation of Connection.compute_window
// (topology.py:348-374) and the layer's step, one launch each per timestep.  The arithmetic is the __host__ __device__ text of
// snn_csrm.hpp (tests/hostcheck/csrm_host.hip runs the same text on the CPU).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_csrm.hpp"

using namespace snn;

// =============================================================================================
// snn_prop_window_f32.  block <-> (column tile of 256, logical slot i, sample b); thread <-> column j.
//  1. the block walks the slot's Nin spike bytes in chunks of 256: every thread reads one byte, the waves compact the spiking
//     indices of the chunk into one ascending list in LDS (wave-64 ballot, popcount below the lane, prefix over the four waves);
//  2. thread j adds W[list[r], j] for r ascending (coalesced across j) -- a silent source's row is never loaded;
//  3. bias, store or accumulate.
// The newest slot (i == W - 1) is read from the source's spike vector itself, never from the ring; its column tile 0 also
// writes that vector over the ring's oldest slot `head`.  Every other slot is read from a ring slot other than `head`, so the
// push has no reader inside the launch.
// =============================================================================================
__global__ __launch_bounds__(256) void k_prop_window(const float *__restrict__ W, const float *__restrict__ bias,
                                                     uint8_t *__restrict__ ring, int head, const uint8_t *__restrict__ s_new,
                                                     float *__restrict__ out, int Wn, int Nin, int N, int accumulate) {
    __shared__ int list[256];
    __shared__ int woff[5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.y, b = blockIdx.z;
    const int j = blockIdx.x * 256 + tid;
    const bool newest = i == Wn - 1;
    const uint8_t *src = newest ? s_new + (size_t)b * Nin : ring + ((size_t)b * Wn + csrm_ring_slot(head, i, Wn)) * Nin;
    uint8_t *push = newest && blockIdx.x == 0 ? ring + ((size_t)b * Wn + head) * Nin : nullptr;
    float acc = 0.0f;
    for (int base = 0; base < Nin; base += 256) {
        const int idx = base + tid;
        const uint8_t sp = idx < Nin ? src[idx] : 0;
        if (push && idx < Nin) push[idx] = sp ? 1 : 0;
        const unsigned long long m = __ballot(sp != 0);
        if (lane == 0) woff[wave + 1] = __popcll(m);
        __syncthreads();
        if (tid == 0) {
            woff[0] = 0;
            for (int w = 0; w < 4; ++w) woff[w + 1] += woff[w];
        }
        __syncthreads();
        if (sp) list[woff[wave] + __popcll(m & ((1ull << lane) - 1ull))] = idx;
        __syncthreads();
        if (j < N) acc = csrm_gather(acc, W, list, woff[4], N, j);
        __syncthreads();                               // the list and the counts are rewritten by the next chunk
    }
    if (j < N) csrm_store(out + ((size_t)b * Wn + i) * N + j, acc, bias, j, accumulate);
}

extern "C" int snn_prop_window_f32(const float *W, const float *bias, uint8_t *ring, int head, const uint8_t *s, float *out,
                                   int B, int Wres, int Nin, int N, int accumulate, snn_stream_t stream) {
    if (!W || !ring || !s || !out || B <= 0 || Wres <= 0 || Nin <= 0 || N <= 0 || head < 0 || head >= Wres) return SNN_ERR_INVALID;
    if (Wres > SNN_CSRM_MAX_WINDOW || B > 65535) return SNN_ERR_UNSUPPORTED;
    if ((long long)B * Wres * N > 2147483647LL || (long long)B * Wres * Nin > 2147483647LL) return SNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_prop_window, dim3((unsigned)((N + 255) / 256), (unsigned)Wres, (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, W, bias, ring, head, s, out, Wres, Nin, N, accumulate);
    return snn_check_launch();
}

// =============================================================================================
// snn_csrm_step.  thread <-> neuron j, looping the batch like k_dc_membrane: theta is shared by the batch and grows by the
// neuron's spike count over the samples.  Element (b, j) owns column j of its sample's rows of `xwin` and `last`.
// =============================================================================================
template <bool PV>
__global__ __launch_bounds__(256) void k_csrm_step(float *__restrict__ v, uint8_t *__restrict__ s, float *__restrict__ x,
                                                   float *__restrict__ theta, const float *__restrict__ xwin,
                                                   float *__restrict__ last, const float *__restrict__ resK, int Wres,
                                                   const float *__restrict__ refK, int Wref, int B, int N, snn_dc_params p,
                                                   uint8_t *__restrict__ raster_s, float *__restrict__ raster_v, snn_pervec pv) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const node_row r = row_of<PV>(p, 0.f, pv, j);
    const float th0 = dc_theta_decayed(theta[j], p.learning, r.theta_decay);   // nodes.py:1438
    const float thr = r.thresh + th0;                                          // nodes.py:1450
    int cnt = 0;
    for (int b = 0; b < B; ++b) {
        const size_t k = (size_t)b * N + j;
        float vv = v[k];
        const uint8_t sp = csrm_update(vv, xwin + (size_t)b * Wres * N + j, last + (size_t)b * Wref * N + j, (size_t)N, resK, Wres,
                                       refK, Wref, thr, r.decay, p.lif);
        v[k] = vv; s[k] = sp;
        cnt += sp;
        if (p.lif.traces) x[k] = trace_next(x[k], sp, r.trace_decay, r.trace_scale, p.lif.traces_additive);
        if (raster_s) raster_s[k] = sp;
        if (raster_v) raster_v[k] = vv;
    }
    theta[j] = dc_theta_bumped(th0, p.learning, r.theta_plus, cnt);            // nodes.py:1453 (the count is exact in f32)
}

extern "C" int snn_csrm_step(float *v, uint8_t *s, float *x, float *theta, const float *xwin, float *last, const float *resK,
                             int Wres, const float *refK, int Wref, int B, int N, const snn_dc_params *h_p, const snn_pervec *pv,
                             uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    if (!v || !s || !theta || !xwin || !last || !resK || !refK || !h_p || B <= 0 || N <= 0 || Wres <= 0 || Wref <= 0) return SNN_ERR_INVALID;
    if (h_p->lif.traces && !x) return SNN_ERR_INVALID;
    if (Wres > SNN_CSRM_MAX_WINDOW || Wref > SNN_CSRM_MAX_WINDOW) return SNN_ERR_UNSUPPORTED;
    if ((long long)B * Wres * N > 2147483647LL || (long long)B * Wref * N > 2147483647LL) return SNN_ERR_UNSUPPORTED;
    const unsigned grid = (unsigned)((N + 255) / 256);
    if (pervec_any(pv)) {
        if (!pervec_within(pv, kPvThresh | kPvTrace | kPvDecay | kPvTheta) || (pv->v[SNN_PV_TRACE_SCALE] && !h_p->lif.traces_additive)) return SNN_ERR_INVALID;
        hipLaunchKernelGGL(k_csrm_step<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, v, s, x, theta, xwin, last, resK, Wres, refK,
                           Wref, B, N, *h_p, raster_s, raster_v, *pv);
    } else
        hipLaunchKernelGGL(k_csrm_step<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, v, s, x, theta, xwin, last, resK, Wres, refK,
                           Wref, B, N, *h_p, raster_s, raster_v, snn_pervec{});
    return snn_check_launch();
}
