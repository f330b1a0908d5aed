// Host-side check of bindsnet_amd/csrc/snn_avgpool.hip: the __host__ __device__ bodies of csrc/snn_avgpool.hpp (avg_geometry,
// avg_window, avg_count, avg_taps / avg_tap_index, avg_value, avg_emit) are run HERE on the CPU, output by output as a kernel
// thread (body 1) or a wave of 64 lanes (body 2) runs them, and compared with F.avg_pool2d by tests/test_avgpool_hostcheck.py.
// Compiled by hipcc like the kernels (same front end, -ffp-contract=off); no device code is executed.  Test infrastructure
// only; not part of libsnnhip.
#include <stdint.h>
#include "../../bindsnet_amd/csrc/snn_avgpool.hpp"

using namespace snn;

// The pooled sizes of a geometry into out_size[2].  Returns 0, or -1 where avg_geometry refuses it.
extern "C" int hostcheck_avgpool_size(const int *in, const int *k, const int *stride, const int *pad, int ceil_mode, int *out_size) {
    AvgGeom g;
    if (!avg_geometry(g, in, k, stride, pad, ceil_mode, 1, 0)) return -1;
    out_size[0] = g.out[0]; out_size[1] = g.out[1];
    return 0;
}

// s [planes, in0, in1] spike bytes, out [planes, out0, out1].  body 1: k_avgpool_thread's loop body per output; body 2:
// k_avgpool_wave's -- 64 lanes take taps lane, lane + 64, ... and their counts are added.  Returns 0, -1 for a refused geometry,
// -2 where an index left the plane (cannot happen: the test's own bound).
extern "C" int hostcheck_avgpool(const uint8_t *s, float *out, long planes, const int *in, const int *k, const int *stride, const int *pad,
                                 int ceil_mode, int include_pad, int divisor, int accumulate, int body) {
    AvgGeom g;
    if (!avg_geometry(g, in, k, stride, pad, ceil_mode, include_pad, divisor)) return -1;
    const long P = avg_plane(g), O = avg_out_plane(g);
    for (long o = 0; o < planes * O; ++o) {
        const long pl = o / O;
        const int oo = (int)(o - pl * O), oh = oo / g.out[1], ow = oo - oh * g.out[1];
        const AvgWindow w = avg_window(g, oh, ow);
        if (w.h0 < 0 || w.w0 < 0 || w.h1 > g.in[0] || w.w1 > g.in[1]) return -2;
        const uint8_t *plane = s + pl * P;
        int c = 0;
        if (body == 2) {
            const int taps = avg_taps(w);
            for (int lane = 0; lane < 64; ++lane)
                for (int t = lane; t < taps; t += 64) {
                    const int i = avg_tap_index(w, t, g.in[1]);
                    if (i < 0 || i >= P) return -2;
                    c += plane[i] != 0;
                }
        } else
            c = avg_count(plane, w, g.in[1]);
        out[o] = avg_emit(avg_value(c, w), accumulate ? out[o] : 0.0f, accumulate);
    }
    return 0;
}
