// snn_pool.hpp -- the order- and rounding-carrying bodies of MaxPool1d / 2d / 3dConnection.compute (bindsnet/network/
// topology.py:1028-1301) and MeanFieldConnection.compute (:1920-2006).
//
// Pooling, per compute(s):
//   fr = fr - f32(decay) * fr        one rounded multiply, one rounded subtract (no FMA: -ffp-contract=off)
//   fr = fr + float(s)               one rounded add
//   indices = F.max_poolNd(fr, kernel, stride, padding, dilation, return_indices=True)[1]
//   out = s.flatten(2).gather(2, indices.flatten(2)).float()
// Index rule of ATen's max_pool kernels (checked against torch in 1, 2 and 3 dimensions, with padding, dilation, ties, NaN
// and all -inf windows: tests/test_pool_hostcheck.py): the window's in-bounds taps are scanned in row-major order; the
// index starts at the first in-bounds tap with the maximum at -inf; a tap replaces the winner iff val > max || isnan(val).
// So the first maximum wins a tie and the last NaN wins.  Indices are flat inside the (b, c) plane.
// One N-d body serves the three ranks: a missing dimension has size 1, kernel 1, stride 1, padding 0, dilation 1.
//
// Mean field: s.float().mean() * w.  The mean of a 0/1 tensor of `numel` <= 2^24 elements is f32(count) / f32(numel), one
// correctly rounded divide (both operands are exact in f32); then one rounded multiply per target and, when accumulating,
// one rounded add.
//
// The bodies are __host__ __device__: tests/hostcheck/pool_host.hip runs them on the CPU against torch and against the
// reference fixtures (tests/test_pool_hostcheck.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snn {

// Geometry of one pooling connection: the (b, c) plane is [in[0], in[1], in[2]] row-major, its pooled plane [out[0], out[1], out[2]].
struct PoolGeom {
    int in[3], out[3], k[3], stride[3], pad[3], dil[3];
};

__host__ __device__ __forceinline__ long pool_plane(const PoolGeom &g) { return (long)g.in[0] * g.in[1] * g.in[2]; }
__host__ __device__ __forceinline__ long pool_out_plane(const PoolGeom &g) { return (long)g.out[0] * g.out[1] * g.out[2]; }

// out_i = (in_i + 2 p_i - d_i (k_i - 1) - 1) / s_i + 1 (floor mode), or 0 where the window does not fit at all.
__host__ __device__ __forceinline__ int pool_out_size(int in, int k, int stride, int pad, int dil) {
    const long span = (long)in + 2L * pad - (long)dil * (k - 1) - 1;
    return span < 0 ? 0 : (int)(span / stride) + 1;
}

// One element's rate update.  `s` is the spike byte.
__host__ __device__ __forceinline__ float pool_rate_next(float fr, float decay, uint8_t s) {
    const float t = decay * fr;
    float r = fr - t;
    r = r + (float)s;
    return r;
}

// First in-bounds tap and the end of the in-bounds taps along one axis of the window of output position o: taps are
// start, start + dil, ... < end.
__host__ __device__ __forceinline__ void pool_axis(int o, int in, int k, int stride, int pad, int dil, int &start, int &end) {
    long s0 = (long)o * stride - pad;
    const long e0 = s0 + (long)(k - 1) * dil + 1;
    while (s0 < 0) s0 += dil;
    start = (int)s0;
    end = (int)(e0 < in ? e0 : in);
}

// Flat index inside the plane `fr` ([in0, in1, in2]) that max_poolNd returns for output position (o0, o1, o2); -1 if the
// window has no in-bounds tap (a dilated window that misses the plane: torch returns an index outside the plane there and the
// reference's gather raises; the Python classes refuse such a geometry; nothing is read here).
__host__ __device__ __forceinline__ int pool_argmax(const float *fr, const PoolGeom &g, int o0, int o1, int o2) {
    int a0, e0, a1, e1, a2, e2;
    pool_axis(o0, g.in[0], g.k[0], g.stride[0], g.pad[0], g.dil[0], a0, e0);
    pool_axis(o1, g.in[1], g.k[1], g.stride[1], g.pad[1], g.dil[1], a1, e1);
    pool_axis(o2, g.in[2], g.k[2], g.stride[2], g.pad[2], g.dil[2], a2, e2);
    if (a0 >= e0 || a1 >= e1 || a2 >= e2) return -1;
    int best = (a0 * g.in[1] + a1) * g.in[2] + a2;
    float mx = -__builtin_inff();
    for (int i0 = a0; i0 < e0; i0 += g.dil[0])
        for (int i1 = a1; i1 < e1; i1 += g.dil[1])
            for (int i2 = a2; i2 < e2; i2 += g.dil[2]) {
                const int idx = (i0 * g.in[1] + i1) * g.in[2] + i2;
                const float v = fr[idx];
                if (v > mx || v != v) { mx = v; best = idx; }
            }
    return best;
}

// The pooled output of flat output position o of one plane: the spike byte at the winning index, as a float.
__host__ __device__ __forceinline__ float pool_gather(const float *fr, const uint8_t *s, const PoolGeom &g, int o) {
    const int o2 = o % g.out[2], r = o / g.out[2];
    const int idx = pool_argmax(fr, g, r / g.out[1], r % g.out[1], o2);
    return idx < 0 ? 0.0f : (float)s[idx];
}

// out (+)= v: a target's summed input takes the term with one rounded add when another connection fed it before.
__host__ __device__ __forceinline__ float pool_emit(float v, float prev, int accumulate) { return accumulate ? prev + v : v; }

// s.float().mean() of a tensor with `count` ones among `numel` <= 2^24 elements.
__host__ __device__ __forceinline__ float meanfield_mean(unsigned count, unsigned numel) { return (float)count / (float)numel; }

// mean * w, added to what the target already holds when accumulating.
__host__ __device__ __forceinline__ float meanfield_emit(float mean, float w, float prev, int accumulate) {
    const float t = mean * w;
    return accumulate ? prev + t : t;
}

}  // namespace snn
