// snn_conversion.hpp -- the arithmetic and the index rule of bindsnet.conversion's layers and connections
// (bindsnet/conversion/nodes.py, topology.py), as __host__ __device__ text: snn_conversion.hip runs it on gfx950,
// tests/hostcheck/conversion_host.hip on the CPU.  Built with -ffp-contract=off: every * + - below is one rounding.
#pragma once
#include <stdint.h>
#include "../../include/snnhip.h"

namespace snn {

// SubtractiveResetIFNodes.forward, bindsnet/conversion/nodes.py:81-97.  The gates are products with 0.0 / 1.0 like the
// reference's `.float() *`, so a zero keeps the sign the product gives it (0.0 * -dt is -0.0, which still counts as
// "not refractory").  The spiking neuron keeps what it holds above the threshold: v - thresh, not a reset value.
__host__ __device__ __forceinline__ uint8_t sif_update(float &v, float &rc, float cur, const snn_lif_params &p) {
    const float gate = (rc == 0.f) ? 1.0f : 0.0f;             // :81  v += (refrac_count == 0).float() * x
    const float gx = gate * cur;
    float vv = v + gx;
    const float live = (rc > 0.f) ? 1.0f : 0.0f;              // :84  (refrac_count > 0).float() * (refrac_count - dt)
    const float down = rc - p.dt;
    float r = live * down;
    const uint8_t sp = vv >= p.thresh;                        // :89
    if (sp) { r = p.refrac; vv = vv - p.thresh; }             // :92-93
    if (p.has_lbound && vv < p.lbound) vv = p.lbound;         // :96-97
    v = vv; rc = r;
    return sp;
}

// Nodes.forward with sum_input, bindsnet/network/nodes.py:109-111: summed += x, the raw input.
__host__ __device__ __forceinline__ float sif_summed(float summed, float cur) { return summed + cur; }

// PassThroughNodes.forward, bindsnet/conversion/nodes.py:169: s = x; as a spike byte, x != 0 (its feeders emit 0.0 or 1.0).
__host__ __device__ __forceinline__ uint8_t pass_spike(float cur) { return cur != 0.f; }

// PermuteConnection / ConstantPad2dConnection.compute as one gather over at most three dimensions (missing leading ones have
// extent 1).  Output element (i0, i1, i2) of a sample reads source element sum_a (i_a - off[a]) * stride[a] where every
// i_a - off[a] lies in [0, src[a]), else nothing (padding: 0).  A permutation has off = 0, src = out and the source's strides
// in the output's order; a padding has the source's own row-major strides and off = the leading pad.
struct GatherGeom { int out[3], src[3], stride[3], off[3]; };

__host__ __device__ __forceinline__ long gather_src(const GatherGeom &g, long j) {
    const int i2 = (int)(j % g.out[2]);
    const long t = j / g.out[2];
    const int i1 = (int)(t % g.out[1]), i0 = (int)(t / g.out[1]);
    const int a0 = i0 - g.off[0], a1 = i1 - g.off[1], a2 = i2 - g.off[2];
    if (a0 < 0 || a0 >= g.src[0] || a1 < 0 || a1 >= g.src[1] || a2 < 0 || a2 >= g.src[2]) return -1;
    return (long)a0 * g.stride[0] + (long)a1 * g.stride[1] + (long)a2 * g.stride[2];
}

__host__ __device__ __forceinline__ float gather_value(const uint8_t *s, const GatherGeom &g, long j) {
    const long i = gather_src(g, j);
    return i < 0 ? 0.0f : (s[i] ? 1.0f : 0.0f);              // .float() of a spike byte
}

// out (+)= v, as snn_prop_pool_f32: one rounded add when another connection fed the target before.
__host__ __device__ __forceinline__ float gather_emit(float v, float prev, int accumulate) { return accumulate ? prev + v : v; }

// The geometry is sound when every extent is positive and the largest source offset an in-range element can reach is
// n_src - 1 at the most: checked on the host before any launch, so the kernel needs no second bound.
inline bool gather_valid(const GatherGeom &g, long n_src, long n_out) {
    long reach = 0, outs = 1;
    for (int a = 0; a < 3; ++a) {
        if (g.out[a] <= 0 || g.src[a] <= 0 || g.stride[a] < 0 || g.off[a] < 0) return false;
        if ((long)g.off[a] + g.src[a] > (long)g.out[a]) return false;       // (no cropping: every source index is some output's)
        reach += (long)(g.src[a] - 1) * g.stride[a];
        outs *= g.out[a];
        if (outs > (1L << 31)) return false;
    }
    return outs == n_out && reach < n_src;
}

}  // namespace snn
