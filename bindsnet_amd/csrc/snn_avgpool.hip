// snn_avgpool.hip -- AvgPool2dConnection.compute on gfx950 (include/snnhip.h, snn_prop_avgpool2d_f32): F.avg_pool2d over 0/1
// spike bytes.  The window rule and the arithmetic are the bodies of snn_avgpool.hpp.
//
// Every output is an integer count of spikes, converted and divided once, so any summation order gives the same bits.  Two
// bodies, chosen by the number of taps kh * kw of a full window:
//   * k_avgpool_thread (fewer than kAvgCoopTaps taps): one output per thread, grid-stride over B * C * OH * OW outputs on at most
//     kAvgMaxGrid workgroups of kAvgThreads threads; consecutive threads take consecutive outputs, so the store is coalesced and
//     neighbouring windows share their cache lines.  The pooling between convolutional layers (2x2, 3x3) runs here.
//   * k_avgpool_wave (kAvgCoopTaps taps and more): one output per WAVE, grid-stride over the outputs on at most kAvgMaxGrid
//     workgroups of kAvgThreads / 64 waves.  Lane l counts taps l, l + 64, ... of the window in row-major order (a whole-plane
//     window is one contiguous run of bytes: 64 consecutive bytes per load), the counts are summed across the lanes with
//     __shfl_xor, and lane 0 writes.  Global pooling -- 32x32 -> 1x1: 1024 taps per output and only B * C outputs -- would leave
//     all but B * C threads idle in the first body and walk 1024 dependent byte loads in each.
// The crossover was measured on the MI355X (profiles/NOTES_avgpool.md; tools/bench_avgpool.py --crossover).
// Every index into a plane is in bounds by construction (avg_axis clips a window to the plane; avg_geometry limits a plane to
// 2^30 elements); the planes and outputs are addressed with size_t.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (csrc/Makefile): the / and the + below are one rounding each.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_avgpool.hpp"

using namespace snn;

namespace {

constexpr int kAvgThreads = 256;
constexpr int kAvgMaxGrid = 1024;
constexpr int kAvgCoopTaps = SNN_AVGPOOL_COOP_TAPS;
constexpr int kWave = 64;

static_assert(kAvgThreads == SNN_AVGPOOL_THREADS && kAvgMaxGrid == SNN_AVGPOOL_MAX_GRID, "the launch limits are part of the documented contract");

int g_body = 0;          // snn_set_avgpool_body: 0 the rule, 1 / 2 one body for every geometry (tests, measurements)

__global__ __launch_bounds__(kAvgThreads) void k_avgpool_thread(const uint8_t *__restrict__ s, float *__restrict__ out, size_t total,
                                                                AvgGeom g, int accumulate) {
    const size_t P = (size_t)avg_plane(g), O = (size_t)avg_out_plane(g);
    for (size_t o = (size_t)blockIdx.x * kAvgThreads + threadIdx.x; o < total; o += (size_t)gridDim.x * kAvgThreads) {
        const size_t pl = o / O;
        const int oo = (int)(o - pl * O), oh = oo / g.out[1], ow = oo - oh * g.out[1];
        const AvgWindow w = avg_window(g, oh, ow);
        const float v = avg_value(avg_count(s + pl * P, w, g.in[1]), w);
        out[o] = avg_emit(v, accumulate ? out[o] : 0.0f, accumulate);
    }
}

__global__ __launch_bounds__(kAvgThreads) void k_avgpool_wave(const uint8_t *__restrict__ s, float *__restrict__ out, size_t total,
                                                              AvgGeom g, int accumulate) {
    const size_t P = (size_t)avg_plane(g), O = (size_t)avg_out_plane(g);
    const int lane = threadIdx.x & (kWave - 1);
    constexpr int waves = kAvgThreads / kWave;
    // (o depends on the wave alone: the loop and the shuffles below are wave-uniform)
    for (size_t o = (size_t)blockIdx.x * waves + (threadIdx.x / kWave); o < total; o += (size_t)gridDim.x * waves) {
        const size_t pl = o / O;
        const int oo = (int)(o - pl * O), oh = oo / g.out[1], ow = oo - oh * g.out[1];
        const AvgWindow w = avg_window(g, oh, ow);
        const uint8_t *plane = s + pl * P;
        const int taps = avg_taps(w);
        int c = 0;
        for (int t = lane; t < taps; t += kWave) c += plane[avg_tap_index(w, t, g.in[1])] != 0;
        for (int d = kWave / 2; d > 0; d >>= 1) c += __shfl_xor(c, d);
        if (lane == 0) out[o] = avg_emit(avg_value(c, w), accumulate ? out[o] : 0.0f, accumulate);
    }
}

}  // namespace

extern "C" void snn_set_avgpool_body(int body) { g_body = body == 1 || body == 2 ? body : 0; }

extern "C" int snn_prop_avgpool2d_f32(const uint8_t *s, float *out, int B, int C, const int *in, const int *k, const int *stride,
                                      const int *pad, int ceil_mode, int count_include_pad, int divisor_override, int accumulate,
                                      snn_stream_t stream) {
    if (!s || !out || B <= 0 || C <= 0) return SNN_ERR_INVALID;
    AvgGeom g;
    if (!avg_geometry(g, in, k, stride, pad, ceil_mode, count_include_pad, divisor_override)) return SNN_ERR_INVALID;
    const long planes = (long)B * C;
    const long P = avg_plane(g), O = avg_out_plane(g);
    if (planes > (1L << 30) || planes * P > (1L << 40) || planes * O > (1L << 40)) return SNN_ERR_UNSUPPORTED;
    const size_t total = (size_t)(planes * O);
    hipStream_t st = (hipStream_t)stream;
    const bool coop = g_body ? g_body == 2 : (long)g.k[0] * g.k[1] >= kAvgCoopTaps;
    if (coop) {
        const long gx = (planes * O + kAvgThreads / kWave - 1) / (kAvgThreads / kWave);
        hipLaunchKernelGGL(k_avgpool_wave, dim3((unsigned)(gx < kAvgMaxGrid ? gx : kAvgMaxGrid)), dim3(kAvgThreads), 0, st, s, out, total, g,
                           accumulate ? 1 : 0);
    } else {
        const long gx = (planes * O + kAvgThreads - 1) / kAvgThreads;
        hipLaunchKernelGGL(k_avgpool_thread, dim3((unsigned)(gx < kAvgMaxGrid ? gx : kAvgMaxGrid)), dim3(kAvgThreads), 0, st, s, out, total, g,
                           accumulate ? 1 : 0);
    }
    return snn_check_launch();
}
