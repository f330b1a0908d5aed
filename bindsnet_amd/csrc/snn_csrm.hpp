// snn_csrm.hpp -- the arithmetic of CSRMNodes (bindsnet/network/nodes.py:1319-1552) and of Connection.compute_window
// (topology.py:348-374) as __host__ __device__ text: snn_csrm.hip launches it, tests/hostcheck/csrm_host.hip runs the same text
// on the CPU.  Built with -ffp-contract=off: every * and + below is one rounding.
//
// The stated order (include/snnhip.h "f13"):
//   window current  x[b,i,j] (+)= ((0 + W[s1,j]) + W[s2,j] + ...) (+ bias[j]),  s1 < s2 < ... the sources that spiked in slot i
//   step            v = v * decay;  res = sum_i resK[i] * x[b,i,j];  ref = sum_i refK[i] * last[b,i,j]  (i ascending from 0.0f,
//                   product then add);  v = v + (res + ref);  s = v >= thresh + theta;  push s into last;  lbound
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"

namespace snn {

// The connection's window of source spikes is a ring of W slots [B, W, Nin] (bytes).  `head` is the physical slot that holds the
// OLDEST entry before a push; the push overwrites it, after which logical slot i (0 = oldest, W - 1 = the vector just pushed)
// is physical slot (head + 1 + i) mod W.
__host__ __device__ __forceinline__ int csrm_ring_slot(int head, int i, int W) {
    int p = head + 1 + i;
    while (p >= W) p -= W;
    return p;
}

// One column's sum over an ascending list of spiking sources, continued from `acc` (0.0f at the start of a slot).
__host__ __device__ __forceinline__ float csrm_gather(float acc, const float *W, const int *list, int k, int N, int j) {
    for (int r = 0; r < k; ++r) acc = acc + W[(size_t)list[r] * N + j];
    return acc;
}

// The finished sum of one (sample, slot, column) into the window-current buffer.
__host__ __device__ __forceinline__ void csrm_store(float *x, float sum, const float *bias, int j, int accumulate) {
    if (bias) sum = sum + bias[j];
    *x = accumulate ? *x + sum : sum;
}

// CSRMNodes.forward for one (sample, neuron), nodes.py:1435-1462, without the batch-shared theta update and the trace.
// x, last: this element's slot 0; consecutive slots are `stride` floats apart.  `last` is shifted by one slot and the new
// spike appended: the element's own column is read and written by this one caller only, each slot read before it is overwritten.
__host__ __device__ __forceinline__ uint8_t csrm_update(float &v, const float *x, float *last, size_t stride, const float *resK,
                                                        int Wres, const float *refK, int Wref, float thr, float decay,
                                                        const snn_lif_params &p) {
    float vv = v * decay;                                   // :1435
    float res = 0.0f;
    for (int i = 0; i < Wres; ++i) {                        // :1441
        const float t = resK[i] * x[(size_t)i * stride];
        res = res + t;
    }
    float ref = 0.0f;
    for (int i = 0; i < Wref; ++i) {                        // :1444
        const float l = last[(size_t)i * stride];
        const float t = refK[i] * l;
        ref = ref + t;
        if (i) last[(size_t)(i - 1) * stride] = l;          // :1456 last_spikes[:, 1:, :] ...
    }
    const float in = res + ref;
    vv = vv + in;                                           // :1447
    const uint8_t sp = vv >= thr;                           // :1450
    last[(size_t)(Wref - 1) * stride] = sp ? 1.0f : 0.0f;   // :1456 ... and s
    if (p.has_lbound && vv < p.lbound) vv = p.lbound;       // :1461
    v = vv;
    return sp;
}

}  // namespace snn
