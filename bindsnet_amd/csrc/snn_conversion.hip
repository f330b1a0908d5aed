// snn_conversion.hip -- bindsnet.conversion on gfx950 (include/snnhip.h f14): the step of SubtractiveResetIFNodes
// (snn_sif_step), of PassThroughNodes (snn_pass_step), and PermuteConnection / ConstantPad2dConnection.compute as one gather
// (snn_prop_gather_f32).  The arithmetic and the index rule are the bodies of snn_conversion.hpp.
//
// All three are pointwise and latency-bound: one grid-stride launch each, state streamed once, every store coalesced (thread
// <-> consecutive output element; the gather's reads are strided bytes of a source that fits in L2).  `summed` is a template
// parameter of the step kernel, so a layer without sum_input compiles to the same loop as before it existed.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (csrc/Makefile): every *, + and - is one rounding.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_conversion.hpp"

using namespace snn;

namespace {

constexpr int kThreads = 256;
constexpr long kMaxGrid = 4096;

unsigned grid_of(long n) { const long g = (n + kThreads - 1) / kThreads; return (unsigned)(g < kMaxGrid ? (g > 0 ? g : 1) : kMaxGrid); }

// PV: per-neuron trace_decay / trace_scale (the only vectors this class reads); the sample is blockIdx.y, as in k_node.
template <bool PV, bool SUM>
__global__ __launch_bounds__(kThreads) void k_sif(float *__restrict__ v, float *__restrict__ refrac, uint8_t *__restrict__ s,
                                                  float *__restrict__ x, float *__restrict__ summed, const float *__restrict__ I,
                                                  long n, snn_lif_params p, uint8_t *__restrict__ raster_s,
                                                  float *__restrict__ raster_v, snn_pervec pv, int N) {
    const long base = PV ? (long)blockIdx.y * N : 0, lim = PV ? (long)N : n;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < lim; j += (long)gridDim.x * blockDim.x) {
        const long k = base + j;
        const node_row r = row_of<PV>(p, 0.f, pv, j);
        float vv = v[k], rc = refrac[k];
        const float cur = I[k];
        const uint8_t sp = sif_update(vv, rc, cur, p);
        v[k] = vv; refrac[k] = rc; s[k] = sp;
        if (p.traces) x[k] = trace_next(x[k], sp, r.trace_decay, r.trace_scale, p.traces_additive);
        if (SUM) summed[k] = sif_summed(summed[k], cur);
        if (raster_s) raster_s[k] = sp;
        if (raster_v) raster_v[k] = vv;
    }
}

__global__ __launch_bounds__(kThreads) void k_pass(uint8_t *__restrict__ s, const float *__restrict__ I, long n,
                                                   uint8_t *__restrict__ raster_s) {
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < n; k += (long)gridDim.x * kThreads) {
        const uint8_t sp = pass_spike(I[k]);
        s[k] = sp;
        if (raster_s) raster_s[k] = sp;
    }
}

__global__ __launch_bounds__(kThreads) void k_gather(const uint8_t *__restrict__ s, float *__restrict__ out, long total, long n_out,
                                                     long n_src, GatherGeom g, int accumulate) {
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < total; k += (long)gridDim.x * kThreads) {
        const long b = k / n_out, j = k - b * n_out;
        const float val = gather_value(s + b * n_src, g, j);
        out[k] = gather_emit(val, accumulate ? out[k] : 0.0f, accumulate);
    }
}

template <bool PV>
void launch_sif(dim3 grid, hipStream_t st, float *v, float *refrac, uint8_t *s, float *x, float *summed, const float *I, long n,
                const snn_lif_params &p, uint8_t *raster_s, float *raster_v, const snn_pervec &pv, int N) {
    if (summed) hipLaunchKernelGGL((k_sif<PV, true>), grid, dim3(kThreads), 0, st, v, refrac, s, x, summed, I, n, p, raster_s, raster_v, pv, N);
    else hipLaunchKernelGGL((k_sif<PV, false>), grid, dim3(kThreads), 0, st, v, refrac, s, x, summed, I, n, p, raster_s, raster_v, pv, N);
}

}  // namespace

extern "C" int snn_sif_step_pv(float *v, float *refrac, uint8_t *s, float *x, float *summed, const float *I, int B, int N,
                               const snn_lif_params *h_p, const snn_pervec *pv, uint8_t *raster_s, float *raster_v,
                               snn_stream_t stream) {
    if (!v || !refrac || !s || !I || !h_p || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (h_p->traces && !x) return SNN_ERR_INVALID;
    const long n = (long)B * N;
    hipStream_t st = (hipStream_t)stream;
    if (pervec_any(pv)) {
        if (!pervec_within(pv, kPvTrace) || !h_p->traces || (pv->v[SNN_PV_TRACE_SCALE] && !h_p->traces_additive)) return SNN_ERR_INVALID;
        if (B > 65535) return SNN_ERR_UNSUPPORTED;
        launch_sif<true>(dim3(grid_of(N), (unsigned)B), st, v, refrac, s, x, summed, I, n, *h_p, raster_s, raster_v, *pv, N);
    } else
        launch_sif<false>(dim3(grid_of(n)), st, v, refrac, s, x, summed, I, n, *h_p, raster_s, raster_v, snn_pervec{}, N);
    return snn_check_launch();
}

extern "C" int snn_sif_step(float *v, float *refrac, uint8_t *s, float *x, float *summed, const float *I, int B, int N,
                            const snn_lif_params *h_p, uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    return snn_sif_step_pv(v, refrac, s, x, summed, I, B, N, h_p, nullptr, raster_s, raster_v, stream);
}

extern "C" int snn_pass_step(uint8_t *s, const float *I, int B, int N, uint8_t *raster_s, snn_stream_t stream) {
    if (!s || !I || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    const long n = (long)B * N;
    hipLaunchKernelGGL(k_pass, dim3(grid_of(n)), dim3(kThreads), 0, (hipStream_t)stream, s, I, n, raster_s);
    return snn_check_launch();
}

extern "C" int snn_prop_gather_f32(const uint8_t *s, float *out, int B, int n_src, const int *out_ext, const int *src_ext,
                                   const int *stride, const int *off, int accumulate, snn_stream_t stream) {
    if (!s || !out || !out_ext || !src_ext || !stride || !off || B <= 0 || n_src <= 0) return SNN_ERR_INVALID;
    GatherGeom g;
    long n_out = 1;
    for (int a = 0; a < 3; ++a) {
        g.out[a] = out_ext[a]; g.src[a] = src_ext[a]; g.stride[a] = stride[a]; g.off[a] = off[a];
        if (out_ext[a] <= 0 || n_out > (1L << 31)) return SNN_ERR_INVALID;
        n_out *= out_ext[a];
    }
    if (!gather_valid(g, n_src, n_out)) return SNN_ERR_INVALID;
    if ((long)B * n_out > (1L << 40) || (long)B * n_src > (1L << 40)) return SNN_ERR_UNSUPPORTED;
    const long total = (long)B * n_out;
    hipLaunchKernelGGL(k_gather, dim3(grid_of(total)), dim3(kThreads), 0, (hipStream_t)stream, s, out, total, n_out, (long)n_src, g,
                       accumulate ? 1 : 0);
    return snn_check_launch();
}
