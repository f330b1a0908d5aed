// snn_real.hpp -- the arithmetic of a real-valued (analog) Input layer and of the two connections that read one
// (include/snnhip.h: snn_prop_dense_real_f32, snn_prop_conv2d_real_f32, snn_input_step_real_pv).  The stated orders of
// snn_prop_dense_f32 / snn_prop_conv2d_f32 / snn_input_step with the spike byte replaced by the f32 value: every multiply and every
// add is rounded on its own (-ffp-contract=off).  __host__ __device__: the kernels of snn_real.hip and the host check
// (tests/hostcheck/real_host.hip) run the same bodies.
#pragma once
#include <hip/hip_runtime.h>

namespace snn {

// one term of a chain: the product rounded, then the add rounded
__host__ __device__ __forceinline__ void real_term(float &acc, float x, float w) {
    const float p = x * w;
    acc = acc + p;
}

// behind the last term: bias (nullable value) last, then out (+)= as in k_prop / k_conv2d -- `(accumulate ? prev : 0) + r`
__host__ __device__ __forceinline__ float real_finish(float acc, bool has_bias, float bias, int accumulate, float prev) {
    float r = acc;
    if (has_bias) r = r + bias;
    return (accumulate ? prev : 0.0f) + r;
}

// Nodes.forward's trace with a real-valued `s` (nodes.py:96-103): x *= trace_decay; set mode -- masked_fill_(s.bool(), trace_scale);
// additive mode -- x += trace_scale * s, the product rounded before the add
__host__ __device__ __forceinline__ float real_trace_next(float x, float s, float decay, float scale, int additive) {
    float t = x * decay;
    if (additive) {
        const float p = scale * s;
        t = t + p;
    } else if (s != 0.0f) t = scale;
    return t;
}

// The chain of one (b, j) of the dense product, source index ascending.  `xv(i)`, `wv(i)`: the sample's value and W[i, j].
// skip_zero: a source whose value is zero is left out (its term is +-0: the same sum for finite weights, the chain starts at +0
// and an f32 sum of finite terms never becomes -0 from there).
template <class X, class Wv>
__host__ __device__ __forceinline__ float real_dense_chain(X xv, Wv wv, int Nin, bool skip_zero) {
    float acc = 0.0f;
    for (int i = 0; i < Nin; ++i) {
        const float x = xv(i);
        if (skip_zero && x == 0.0f) continue;
        real_term(acc, x, wv(i));
    }
    return acc;
}

// The chains of U output channels of one output pixel (oy, ox): taps row-major, input channel innermost, out-of-image taps
// skipped.  `img(ci, iy, ix)`: the sample's value; `wt(u, ci, ky, kx)`: the weight of the thread's u-th channel (0 for a channel
// beyond Cout: its chain is never stored).  A zero value is skipped as in k_conv2d (a +-0 term).
template <int U, class Img, class Wt>
__host__ __device__ __forceinline__ void real_conv2d_chains(float (&acc)[U], Img img, Wt wt, int Cin, int H, int Wd, int KH, int KW,
                                                           int stride, int pad, int oy, int ox) {
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.0f;
    for (int ky = 0; ky < KH; ++ky) {
        const int iy = oy * stride - pad + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < KW; ++kx) {
            const int ix = ox * stride - pad + kx;
            if (ix < 0 || ix >= Wd) continue;
            for (int ci = 0; ci < Cin; ++ci) {
                const float x = img(ci, iy, ix);
                if (x == 0.0f) continue;
#pragma unroll
                for (int u = 0; u < U; ++u) real_term(acc[u], x, wt(u, ci, ky, kx));
            }
        }
    }
}

}  // namespace snn
