// snn_pool.hip -- MaxPool1d / 2d / 3dConnection.compute and MeanFieldConnection.compute on gfx950 (include/snnhip.h,
// snn_prop_pool_f32 / snn_prop_meanfield_f32).  The arithmetic and the index rule are the bodies of snn_pool.hpp.
//
// Pooling reads the UPDATED rates of overlapping windows, so the rate update and the pooling of one (b, c) plane cannot be
// one elementwise pass.  Two forms, the same bodies and so the same bits:
//   * staged (one launch): a plane of at most kPoolStage = 8192 elements.  A workgroup of 256 threads takes G consecutive
//     planes (G * plane <= kPoolStage), updates their rates into LDS (32 KiB of rates + 8 KiB of spike bytes), writes them
//     back once, and pools from LDS after one barrier.  G = min(kPoolStage / plane, ceil(planes / kPoolMaxGrid)), at least 1;
//     the grid is min(ceil(planes / G), kPoolMaxGrid) workgroups striding over the plane groups.
//   * global (two launches): a plane of more than kPoolStage elements.  k_pool_rates updates every rate in place, k_pool_global
//     pools from global memory, one thread per output, both grid-stride over at most kPoolMaxGrid workgroups.
// Every index into a plane is bounds-checked by construction (pool_axis clips a window to the plane); a window without an
// in-bounds tap (a dilated window that misses the plane; the Python classes refuse it) reads nothing and yields 0.
//
// Mean field: one launch, no host synchronisation.  Every workgroup (at most kMeanMaxGrid = 64 of 256 threads) counts the
// spikes of the WHOLE [B, n_src] tensor itself -- integer adds, four bytes per load where the pointer allows, a wave
// reduction and four partial counts through LDS -- forms the mean and then writes its share of the B * n_tgt outputs.
// Counting again per workgroup costs B * n_src bytes of cached reads each and saves a second launch and a counter that would
// have to be zeroed; the generic plan is launch-bound.  The price grows with the source tensor: a thread walks B * n_src / 1024
// dependent loads before the first output is written, 16 K of them at the accepted maximum of 2^24 bytes, so a mean field
// over millions of source elements is slow (per-call times by size: profiles/NOTES_pool.md; tools/bench_pool.py --meanfield).
// It is meant for layers of up to some 10^5 neurons x batch; a two-launch count is the follow-up if larger ones matter.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (csrc/Makefile): every *, +, - and / below is one rounding.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_pool.hpp"

using namespace snn;

namespace {

constexpr int kPoolThreads = 256;
constexpr int kPoolStage = 8192;            // elements of one workgroup's staged planes
constexpr int kPoolMaxGrid = 1024;
constexpr int kMeanThreads = 256;
constexpr int kMeanMaxGrid = 64;

static_assert(kPoolStage == SNN_POOL_STAGE, "the staging limit is part of the documented contract");

__global__ __launch_bounds__(kPoolThreads) void k_pool_staged(float *__restrict__ fr, const uint8_t *__restrict__ s,
                                                              float *__restrict__ out, long planes, int G, PoolGeom g,
                                                              float decay, int accumulate) {
    __shared__ float rates[kPoolStage];
    __shared__ uint8_t spikes[kPoolStage];
    const int P = (int)pool_plane(g), O = (int)pool_out_plane(g);
    const long groups = (planes + G - 1) / G;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long p0 = grp * G;
        const int np = (int)(planes - p0 < G ? planes - p0 : G);
        const size_t base = (size_t)p0 * P;
        const int n = np * P;                                   // <= kPoolStage
        for (int i = threadIdx.x; i < n; i += kPoolThreads) {
            const uint8_t sv = s[base + i];
            const float r = pool_rate_next(fr[base + i], decay, sv);
            rates[i] = r;
            spikes[i] = sv;
            fr[base + i] = r;
        }
        __syncthreads();
        const size_t obase = (size_t)p0 * O;
        const long no = (long)np * O;
        for (long o = threadIdx.x; o < no; o += kPoolThreads) {
            const int pl = (int)(o / O), oo = (int)(o - (long)pl * O);
            const float v = pool_gather(rates + pl * P, spikes + pl * P, g, oo);
            float *dst = out + obase + o;
            *dst = pool_emit(v, accumulate ? *dst : 0.0f, accumulate);
        }
        __syncthreads();                                        // the next group's staging overwrites what was just read
    }
}

__global__ __launch_bounds__(kPoolThreads) void k_pool_rates(float *__restrict__ fr, const uint8_t *__restrict__ s, size_t n,
                                                             float decay) {
    for (size_t i = (size_t)blockIdx.x * kPoolThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kPoolThreads)
        fr[i] = pool_rate_next(fr[i], decay, s[i]);
}

__global__ __launch_bounds__(kPoolThreads) void k_pool_global(const float *__restrict__ fr, const uint8_t *__restrict__ s,
                                                              float *__restrict__ out, long planes, PoolGeom g, int accumulate) {
    const size_t P = (size_t)pool_plane(g), O = (size_t)pool_out_plane(g), n = (size_t)planes * O;
    for (size_t o = (size_t)blockIdx.x * kPoolThreads + threadIdx.x; o < n; o += (size_t)gridDim.x * kPoolThreads) {
        const size_t pl = o / O;
        const float v = pool_gather(fr + pl * P, s + pl * P, g, (int)(o - pl * O));
        out[o] = pool_emit(v, accumulate ? out[o] : 0.0f, accumulate);
    }
}

__global__ __launch_bounds__(kMeanThreads) void k_meanfield(const float *__restrict__ w, unsigned w_numel, const uint8_t *__restrict__ s,
                                                            float *__restrict__ out, unsigned numel, size_t n_out, int mode) {
    __shared__ unsigned part[kMeanThreads / 64];
    const unsigned tid = threadIdx.x;
    // the bytes before the first 4-byte boundary, the aligned words, the bytes behind the last whole word
    unsigned head = (unsigned)((4u - ((uintptr_t)s & 3u)) & 3u);
    if (head > numel) head = numel;
    const unsigned words = (numel - head) / 4u, tail0 = head + 4u * words;
    unsigned c = 0;
    if (tid < head) c += s[tid];
    const uint32_t *sw = (const uint32_t *)(s + head);
    for (unsigned i = tid; i < words; i += kMeanThreads) {
        const uint32_t v = sw[i];
        c += (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24);
    }
    if (tail0 + tid < numel) c += s[tail0 + tid];               // at most three bytes
    for (int d = 32; d > 0; d >>= 1) c += (unsigned)__shfl_xor((int)c, d);
    if ((tid & 63u) == 0) part[tid >> 6] = c;
    __syncthreads();
    unsigned count = 0;
#pragma unroll
    for (int k = 0; k < kMeanThreads / 64; ++k) count += part[k];
    const float mean = meanfield_mean(count, numel);
    for (size_t o = (size_t)blockIdx.x * kMeanThreads + tid; o < n_out; o += (size_t)gridDim.x * kMeanThreads) {
        const float wv = w[w_numel == 1 ? 0 : o % w_numel];
        if (mode == SNN_MEANFIELD_STORE) out[o] = meanfield_emit(mean, wv, 0.0f, 0);
        else out[o] = meanfield_emit(mean, wv, mode ? out[o] : 0.0f, 1);
    }
}

int pool_geometry(PoolGeom &g, const int *in, const int *k, const int *stride, const int *pad, const int *dil) {
    if (!in || !k || !stride || !pad || !dil) return SNN_ERR_INVALID;
    for (int a = 0; a < 3; ++a) {
        if (in[a] <= 0 || k[a] <= 0 || stride[a] <= 0 || pad[a] < 0 || dil[a] <= 0) return SNN_ERR_INVALID;
        if ((long)dil[a] * (k[a] - 1) + 1 > 2147483647L) return SNN_ERR_INVALID;
        if (2L * pad[a] > (long)dil[a] * (k[a] - 1) + 1) return SNN_ERR_INVALID;    // torch: at most half of the effective kernel
        g.in[a] = in[a]; g.k[a] = k[a]; g.stride[a] = stride[a]; g.pad[a] = pad[a]; g.dil[a] = dil[a];
        g.out[a] = pool_out_size(in[a], k[a], stride[a], pad[a], dil[a]);
        if (g.out[a] <= 0) return SNN_ERR_INVALID;
    }
    return SNN_OK;
}

}  // namespace

extern "C" int snn_prop_pool_f32(float *fr, const uint8_t *s, float *out, int B, int C, const int *in, const int *k,
                                 const int *stride, const int *pad, const int *dil, float decay, int accumulate,
                                 snn_stream_t stream) {
    if (!fr || !s || !out || B <= 0 || C <= 0) return SNN_ERR_INVALID;
    PoolGeom g;
    const int rc = pool_geometry(g, in, k, stride, pad, dil);
    if (rc != SNN_OK) return rc;
    const long planes = (long)B * C;
    const long P = pool_plane(g), O = pool_out_plane(g);
    if (P > (1L << 30) || O > (1L << 30) || planes > (1L << 30) || planes * P > (1L << 40) || planes * O > (1L << 40))
        return SNN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (P <= kPoolStage) {
        long G = kPoolStage / P;
        const long spread = (planes + kPoolMaxGrid - 1) / kPoolMaxGrid;
        if (G > spread) G = spread;
        if (G < 1) G = 1;
        const long groups = (planes + G - 1) / G;
        hipLaunchKernelGGL(k_pool_staged, dim3((unsigned)(groups < kPoolMaxGrid ? groups : kPoolMaxGrid)), dim3(kPoolThreads), 0, st,
                           fr, s, out, planes, (int)G, g, decay, accumulate ? 1 : 0);
        return snn_check_launch();
    }
    const long ge = (planes * P + kPoolThreads - 1) / kPoolThreads, go = (planes * O + kPoolThreads - 1) / kPoolThreads;
    hipLaunchKernelGGL(k_pool_rates, dim3((unsigned)(ge < kPoolMaxGrid ? ge : kPoolMaxGrid)), dim3(kPoolThreads), 0, st, fr, s,
                       (size_t)(planes * P), decay);
    hipLaunchKernelGGL(k_pool_global, dim3((unsigned)(go < kPoolMaxGrid ? go : kPoolMaxGrid)), dim3(kPoolThreads), 0, st, fr, s, out,
                       planes, g, accumulate ? 1 : 0);
    return snn_check_launch();
}

extern "C" int snn_prop_meanfield_f32(const float *w, int w_numel, const uint8_t *s, float *out, int B, int n_src, int n_tgt,
                                      int accumulate, snn_stream_t stream) {
    if (!w || !s || !out || B <= 0 || n_src <= 0 || n_tgt <= 0 || w_numel <= 0 || accumulate < 0 || accumulate > SNN_MEANFIELD_STORE)
        return SNN_ERR_INVALID;
    const long numel = (long)B * n_src, n_out = (long)B * n_tgt;
    if (n_out % w_numel != 0) return SNN_ERR_INVALID;
    if (numel > (1L << 24)) return SNN_ERR_UNSUPPORTED;          // f32(count) and f32(numel) are exact up to here
    const long gx = (n_out + kMeanThreads - 1) / kMeanThreads;
    hipLaunchKernelGGL(k_meanfield, dim3((unsigned)(gx < kMeanMaxGrid ? gx : kMeanMaxGrid)), dim3(kMeanThreads), 0, (hipStream_t)stream,
                       w, (unsigned)w_numel, s, out, (unsigned)numel, (size_t)n_out, accumulate);
    return snn_check_launch();
}
