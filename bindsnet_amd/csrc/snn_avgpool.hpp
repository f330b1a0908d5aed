// snn_avgpool.hpp -- the window rule and the arithmetic of AvgPool2dConnection.compute, which is
//   F.avg_pool2d(s.float(), kernel_size, stride, padding, ceil_mode, count_include_pad, divisor_override)
// over 0/1 spikes.  Not in the reference; the oracle is ATen's avg_pool2d on the CPU, whose rule this restates:
//   out size   o = floor((in + 2 p - k + (ceil_mode ? stride - 1 : 0)) / stride) + 1, and with ceil_mode one less where the last
//              window would start at or behind in + p (in the right padding or past it)
//   window     [o * stride - p, min(o * stride - p + k, in + p)) per axis: clipped to the PADDED plane -- pool_size is the product
//              of the two lengths --, then clipped to the plane itself: the in-plane taps
//   divisor    divisor_override where given, else pool_size (count_include_pad) or the number of in-plane taps
//   value      sum of the in-plane taps / divisor; 0 where the window has no in-plane tap
// The taps are 0 or 1, so the sum is an integer count: whatever order it is taken in, f32(count) is the same exact float
// (a window has far fewer than 2^24 taps), and count / divisor is ONE correctly rounded IEEE division, as ATen's.  That is why the
// two bodies of snn_avgpool.hip, and any thread count of torch's, give the same bits.
//
// The bodies are __host__ __device__: tests/hostcheck/avgpool_host.hip runs them on the CPU against torch
// (tests/test_avgpool_hostcheck.py).  Built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snn {

// One average pooling: the (b, c) plane is [in[0], in[1]] row-major, its pooled plane [out[0], out[1]].  divisor 0: none given.
struct AvgGeom {
    int in[2], out[2], k[2], stride[2], pad[2];
    int include_pad, divisor;
};

// One output's window: the in-plane taps are rows [h0, h1) x columns [w0, w1) (empty where h0 >= h1 or w0 >= w1), div its divisor.
struct AvgWindow {
    int h0, h1, w0, w1, div;
};

__host__ __device__ __forceinline__ long avg_plane(const AvgGeom &g) { return (long)g.in[0] * g.in[1]; }
__host__ __device__ __forceinline__ long avg_out_plane(const AvgGeom &g) { return (long)g.out[0] * g.out[1]; }

// ATen's pooling_output_shape at dilation 1; 0 or less where no window fits.
__host__ __device__ __forceinline__ long avg_out_size(int in, int k, int stride, int pad, int ceil_mode) {
    const long num = (long)in + 2L * pad - k + (ceil_mode ? stride - 1 : 0);
    long o = (num >= 0 ? num / stride : -((-num + stride - 1) / stride)) + 1;      // floor division
    if (ceil_mode && (o - 1) * stride >= (long)in + pad) --o;
    return o;
}

// One axis of output position o: the length of the window clipped to the padded plane, and its in-plane part [a, e).
__host__ __device__ __forceinline__ int avg_axis(int o, int in, int k, int stride, int pad, int &a, int &e) {
    const long s0 = (long)o * stride - pad;
    long e0 = s0 + k;
    if (e0 > (long)in + pad) e0 = (long)in + pad;
    a = (int)(s0 < 0 ? 0 : s0);
    e = (int)(e0 < in ? e0 : in);
    return (int)(e0 - s0);
}

__host__ __device__ __forceinline__ AvgWindow avg_window(const AvgGeom &g, int oh, int ow) {
    AvgWindow w;
    const int lh = avg_axis(oh, g.in[0], g.k[0], g.stride[0], g.pad[0], w.h0, w.h1);
    const int lw = avg_axis(ow, g.in[1], g.k[1], g.stride[1], g.pad[1], w.w0, w.w1);
    const bool empty = w.h0 >= w.h1 || w.w0 >= w.w1;
    w.div = g.divisor ? g.divisor : g.include_pad ? lh * lw : empty ? 1 : (w.h1 - w.h0) * (w.w1 - w.w0);
    return w;
}

__host__ __device__ __forceinline__ bool avg_empty(const AvgWindow &w) { return w.h0 >= w.h1 || w.w0 >= w.w1; }

// The in-plane taps of a window, and tap t of them in row-major order as an index into the plane.
__host__ __device__ __forceinline__ int avg_taps(const AvgWindow &w) { return avg_empty(w) ? 0 : (w.h1 - w.h0) * (w.w1 - w.w0); }
__host__ __device__ __forceinline__ int avg_tap_index(const AvgWindow &w, int t, int in_w) {
    const int ww = w.w1 - w.w0, r = t / ww;
    return (w.h0 + r) * in_w + w.w0 + (t - r * ww);
}

// The spikes among the in-plane taps, one after the other: what one thread of the per-output body counts.
__host__ __device__ __forceinline__ int avg_count(const uint8_t *plane, const AvgWindow &w, int in_w) {
    int c = 0;
    for (int h = w.h0; h < w.h1; ++h)
        for (int x = w.w0; x < w.w1; ++x) c += plane[h * in_w + x] != 0;
    return c;
}

// count -> value: exact conversions, one rounded division.  A window without an in-plane tap is 0, whatever its divisor.
__host__ __device__ __forceinline__ float avg_value(int count, const AvgWindow &w) {
    return avg_empty(w) ? 0.0f : (float)count / (float)w.div;
}

// out (+)= v, as snn_prop_local_f32: one rounded add when another connection fed the target before.
__host__ __device__ __forceinline__ float avg_emit(float v, float prev, int accumulate) { return accumulate ? prev + v : v; }

// The geometry of the arguments of snn_prop_avgpool2d_f32, or false where ATen refuses it too (a pad beyond half the kernel, a
// zero divisor is "none given" here) or no window fits.  Every index the bodies form lies inside the plane by construction of
// avg_axis (0 <= a, e <= in); nothing else is needed for the bounds.
inline bool avg_geometry(AvgGeom &g, const int *in, const int *k, const int *stride, const int *pad, int ceil_mode, int include_pad,
                         int divisor) {
    if (!in || !k || !stride || !pad) return false;
    for (int a = 0; a < 2; ++a) {
        if (in[a] <= 0 || k[a] <= 0 || stride[a] <= 0 || pad[a] < 0 || 2L * pad[a] > k[a]) return false;
        if (in[a] > (1 << 30) || k[a] > (1 << 30) || stride[a] > (1 << 30)) return false;
        const long o = avg_out_size(in[a], k[a], stride[a], pad[a], ceil_mode);
        if (o <= 0 || o > (1L << 30)) return false;
        g.in[a] = in[a]; g.k[a] = k[a]; g.stride[a] = stride[a]; g.pad[a] = pad[a]; g.out[a] = (int)o;
    }
    if ((long)g.k[0] * g.k[1] > (1L << 24)) return false;         // f32(count) and f32(pool_size) stay exact
    if (avg_plane(g) > (1L << 30) || avg_out_plane(g) > (1L << 30)) return false;      // indices into a plane are ints
    g.include_pad = include_pad ? 1 : 0;
    g.divisor = divisor;
    return true;
}

}  // namespace snn
