// snn_nodes.hip -- step kernels of the node layers beyond LIF / Diehl&Cook: McCullochPitts, IFNodes, BoostedLIFNodes,
// CurrentLIFNodes, IzhikevichNodes (bindsnet/network/nodes.py:231, :308, :562, :681, :1147) + their C-ABI entry points.
// One launch per layer per timestep; every kernel writes the layer's monitor slices itself.  The arithmetic is the
// __host__ __device__ text of snn_common.hpp (tests/hostcheck/nodes_host.hip runs the same text on the CPU).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_order.hpp"
#include "snn_common.hpp"

using namespace snn;

// =============================================================================================
// Pointwise layers: grid-stride over B*N, state streamed once (like k_lif of snn_ops.hip).
// =============================================================================================
enum { kMcp = 0, kIf = 1, kBoosted = 2, kClif = 3 };

// PV: the instance for layers with per-neuron parameters (snn_pervec).  Its grid is (blocks over the N neurons, B samples): the
// loop runs over the neuron j of sample blockIdx.y, so row j of the [N] vectors is loaded without a division, coalesced, and
// the B blocks of a column range re-read it from L2.  The scalar instance walks the flat B*N range exactly as before.
template <int KIND, bool PV>
__global__ __launch_bounds__(256) void k_node(float *__restrict__ v, float *__restrict__ refrac, float *__restrict__ aux,
                                              uint8_t *__restrict__ s, float *__restrict__ x, float *__restrict__ I, long n,
                                              snn_lif_params p, float aux_decay, uint8_t *__restrict__ raster_s,
                                              float *__restrict__ raster_v, snn_pervec pv, int N) {
    const long base = PV ? (long)blockIdx.y * N : 0, lim = PV ? (long)N : n;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < lim; j += (long)gridDim.x * blockDim.x) {
        const long k = base + j;
        const node_row r = row_of<PV>(p, aux_decay, pv, j);
        float vv = v[k], cur = I[k];
        uint8_t sp;
        if (KIND == kMcp) {
            sp = mcp_update(vv, cur, r.thresh);
        } else {
            float rc = refrac[k];
            if (KIND == kIf) sp = if_update(vv, rc, cur, p, r.thresh);
            else if (KIND == kBoosted) {
                if (rc > 0.f) { cur = 0.f; I[k] = 0.f; }      // nodes.py:633 masks the caller's tensor in place
                sp = boosted_update(vv, rc, cur, p, r.thresh, r.decay);
            } else {
                float ii = aux[k];
                sp = clif_update(vv, rc, ii, cur, r.i_decay, p, r.thresh, r.decay);
                aux[k] = ii;
            }
            refrac[k] = rc;
        }
        v[k] = vv; s[k] = sp;
        if (p.traces) x[k] = trace_next(x[k], sp, r.trace_decay, r.trace_scale, p.traces_additive);
        if (raster_s) raster_s[k] = sp;
        if (raster_v) raster_v[k] = vv;
    }
}

template <int KIND>
static int launch_node(float *v, float *refrac, float *aux, uint8_t *s, float *x, float *I, int B, int N,
                       const snn_lif_params *h_p, float aux_decay, const snn_pervec *pv, uint8_t *raster_s, float *raster_v,
                       snn_stream_t stream) {
    if (!v || !s || !I || !h_p || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (KIND != kMcp && !refrac) return SNN_ERR_INVALID;
    if (KIND == kClif && !aux) return SNN_ERR_INVALID;
    if (h_p->traces && !x) return SNN_ERR_INVALID;
    const long n = (long)B * N;
    if (pervec_any(pv)) {
        const unsigned allowed = kPvThresh | kPvTrace | (KIND == kBoosted || KIND == kClif ? kPvDecay : 0u) | (KIND == kClif ? kPvIDecay : 0u);
        if (!pervec_within(pv, allowed) || (pv->v[SNN_PV_TRACE_SCALE] && !h_p->traces_additive)) return SNN_ERR_INVALID;
        if (B > 65535) return SNN_ERR_UNSUPPORTED;
        const unsigned gx = (unsigned)((N + 255) / 256 < 4096 ? (N + 255) / 256 : 4096);
        hipLaunchKernelGGL((k_node<KIND, true>), dim3(gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, v, refrac, aux, s, x, I, n, *h_p,
                           aux_decay, raster_s, raster_v, *pv, N);
        return snn_check_launch();
    }
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL((k_node<KIND, false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, v, refrac, aux, s, x, I, n, *h_p, aux_decay,
                       raster_s, raster_v, snn_pervec{}, N);
    return snn_check_launch();
}

extern "C" int snn_mcp_step_pv(float *v, uint8_t *s, float *x, const float *I, int B, int N, const snn_lif_params *h_p,
                               const snn_pervec *pv, uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    return launch_node<kMcp>(v, nullptr, nullptr, s, x, const_cast<float *>(I), B, N, h_p, 0.f, pv, raster_s, raster_v, stream);
}
extern "C" int snn_mcp_step(float *v, uint8_t *s, float *x, const float *I, int B, int N, const snn_lif_params *h_p,
                            uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    return snn_mcp_step_pv(v, s, x, I, B, N, h_p, nullptr, raster_s, raster_v, stream);
}

extern "C" int snn_if_step_pv(float *v, float *refrac, uint8_t *s, float *x, const float *I, int B, int N,
                              const snn_lif_params *h_p, const snn_pervec *pv, uint8_t *raster_s, float *raster_v,
                              snn_stream_t stream) {
    return launch_node<kIf>(v, refrac, nullptr, s, x, const_cast<float *>(I), B, N, h_p, 0.f, pv, raster_s, raster_v, stream);
}
extern "C" int snn_if_step(float *v, float *refrac, uint8_t *s, float *x, const float *I, int B, int N,
                           const snn_lif_params *h_p, uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    return snn_if_step_pv(v, refrac, s, x, I, B, N, h_p, nullptr, raster_s, raster_v, stream);
}

extern "C" int snn_boosted_step_pv(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N,
                                   const snn_lif_params *h_p, const snn_pervec *pv, uint8_t *raster_s, float *raster_v,
                                   snn_stream_t stream) {
    return launch_node<kBoosted>(v, refrac, nullptr, s, x, I, B, N, h_p, 0.f, pv, raster_s, raster_v, stream);
}
extern "C" int snn_boosted_step(float *v, float *refrac, uint8_t *s, float *x, float *I, int B, int N,
                                const snn_lif_params *h_p, uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    return snn_boosted_step_pv(v, refrac, s, x, I, B, N, h_p, nullptr, raster_s, raster_v, stream);
}

extern "C" int snn_clif_step_pv(float *v, float *refrac, float *i, uint8_t *s, float *x, const float *I, int B, int N,
                                const snn_lif_params *h_p, float i_decay, const snn_pervec *pv, uint8_t *raster_s,
                                float *raster_v, snn_stream_t stream) {
    return launch_node<kClif>(v, refrac, i, s, x, const_cast<float *>(I), B, N, h_p, i_decay, pv, raster_s, raster_v, stream);
}
extern "C" int snn_clif_step(float *v, float *refrac, float *i, uint8_t *s, float *x, const float *I, int B, int N,
                             const snn_lif_params *h_p, float i_decay, uint8_t *raster_s, float *raster_v,
                             snn_stream_t stream) {
    return snn_clif_step_pv(v, refrac, i, s, x, I, B, N, h_p, i_decay, nullptr, raster_s, raster_v, stream);
}

// =============================================================================================
// Izhikevich: the whole step in one launch.  block <-> sample b, thread <-> neuron j (blockDim = N rounded up to whole
// waves, at most SNN_IZH_MAX_N).
//  1. every thread reads its own entry spike s[b,j]; the waves compact the spiking indices into one ascending list in LDS
//     (wave-64 ballot, popcount below the lane, prefix over the waves' counts).
//  2. thread j walks the list in rank order: term r is St[list[r], j] (coalesced across j), fed through inner_sum8_terms --
//     ATen's order for S[:, s[b]].sum(dim=1) over the k selected columns.
//  3. izh_update, trace, rasters.
// The entry spikes are read only in step 1, and the list is complete (third barrier) before any thread stores a new s: no
// separate entry copy is needed.
// =============================================================================================
template <bool PV>
__global__ __launch_bounds__(SNN_IZH_MAX_N) void k_izh(float *__restrict__ v, float *__restrict__ u, uint8_t *__restrict__ s,
                                                       float *__restrict__ x, float *__restrict__ I,
                                                       const float *__restrict__ a, const float *__restrict__ b,
                                                       const float *__restrict__ c, const float *__restrict__ d,
                                                       const float *__restrict__ St, int N, snn_lif_params p,
                                                       uint8_t *__restrict__ raster_s, float *__restrict__ raster_v,
                                                       snn_pervec pv) {
    __shared__ int list[SNN_IZH_MAX_N];
    __shared__ int woff[SNN_IZH_MAX_N / 64 + 1];
    const int j = threadIdx.x, lane = j & 63, wave = j >> 6, nw = blockDim.x >> 6;
    const size_t base = (size_t)blockIdx.x * N;
    const uint8_t sj = j < N ? s[base + j] : 0;
    const unsigned long long m = __ballot(sj != 0);
    if (lane == 0) woff[wave + 1] = __popcll(m);
    __syncthreads();
    if (j == 0) {
        woff[0] = 0;
        for (int w = 0; w < nw; ++w) woff[w + 1] += woff[w];
    }
    __syncthreads();
    if (sj) list[woff[wave] + __popcll(m & ((1ull << lane) - 1ull))] = j;
    __syncthreads();
    const int k = woff[nw];
    if (j >= N) return;
    const float lat = inner_sum8_terms([&](int r) { return St[(size_t)list[r] * N + j]; }, k);
    const float cur = I[base + j] + lat;           // nodes.py:1279 x += ...
    I[base + j] = cur;
    float vv = v[base + j], uu = u[base + j];
    const node_row r = row_of<PV>(p, 0.f, pv, j);      // (thread <-> neuron: row j beside a[j] .. d[j])
    const uint8_t sp = izh_update(vv, uu, sj, cur, a[j], b[j], c[j], d[j], p, r.thresh);
    v[base + j] = vv; u[base + j] = uu; s[base + j] = sp;
    if (p.traces) x[base + j] = trace_next(x[base + j], sp, r.trace_decay, r.trace_scale, p.traces_additive);
    if (raster_s) raster_s[base + j] = sp;
    if (raster_v) raster_v[base + j] = vv;
}

extern "C" int snn_izh_step_pv(float *v, float *u, uint8_t *s, float *x, float *I, const float *a, const float *b, const float *c,
                               const float *d, const float *St, int B, int N, const snn_lif_params *h_p, const snn_pervec *pv,
                               uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    if (!v || !u || !s || !I || !a || !b || !c || !d || !St || !h_p || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (h_p->traces && !x) return SNN_ERR_INVALID;
    if (N > SNN_IZH_MAX_N) return SNN_ERR_UNSUPPORTED;
    const unsigned threads = (unsigned)((N + 63) / 64) * 64;
    if (pervec_any(pv)) {
        if (!pervec_within(pv, kPvThresh | kPvTrace) || (pv->v[SNN_PV_TRACE_SCALE] && !h_p->traces_additive)) return SNN_ERR_INVALID;
        hipLaunchKernelGGL(k_izh<true>, dim3((unsigned)B), dim3(threads), 0, (hipStream_t)stream, v, u, s, x, I, a, b, c, d, St, N, *h_p,
                           raster_s, raster_v, *pv);
    } else
        hipLaunchKernelGGL(k_izh<false>, dim3((unsigned)B), dim3(threads), 0, (hipStream_t)stream, v, u, s, x, I, a, b, c, d, St, N, *h_p,
                           raster_s, raster_v, snn_pervec{});
    return snn_check_launch();
}
extern "C" int snn_izh_step(float *v, float *u, uint8_t *s, float *x, float *I, const float *a, const float *b, const float *c,
                            const float *d, const float *St, int B, int N, const snn_lif_params *h_p, uint8_t *raster_s,
                            float *raster_v, snn_stream_t stream) {
    return snn_izh_step_pv(v, u, s, x, I, a, b, c, d, St, B, N, h_p, nullptr, raster_s, raster_v, stream);
}
