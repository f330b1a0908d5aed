// snn_synparams.hpp -- the per-element arithmetic of the dense learning rules with per-synapse constants (include/snnhip.h f13).
//
// The *_pv instances of the update kernels in snn_ops.hip read every weight element's learning rates and bounds through
// syn_at() and finish through the bodies below; tests/hostcheck/synparams_host.hip compiles the same bodies for the CPU and drives
// them element by element against reference fixtures (tests/test_synparams_hostcheck.py).  Built with -ffp-contract=off: every
// operation below is one rounding, in the reference's order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/snnhip.h"

namespace snn {

// One constant of a weight element: the tensor's entry for (source s, target n), or the scalar where no tensor is named.
__host__ __device__ __forceinline__ float syn_at(const float *p, int rs, int cs, float scalar, int s, int n) {
    return p ? p[(long)s * rs + (long)n * cs] : scalar;
}

// The four constants of element (s, n).  `wmin` / `wmax` are -inf / +inf where the scalar bound is absent.
struct SynElem { float nu0, nu1, lo, hi; };
__host__ __device__ __forceinline__ SynElem syn_elem(const snn_synparams &q, float nu0, float nu1, int has_min, float wmin, int has_max,
                                                     float wmax, int s, int n) {
    SynElem e;
    e.nu0 = syn_at(q.nu0, q.nu0_rs, q.nu0_cs, nu0, s, n);
    e.nu1 = syn_at(q.nu1, q.nu1_rs, q.nu1_cs, nu1, s, n);
    e.lo = syn_at(q.wmin, q.wmin_rs, q.wmin_cs, has_min ? wmin : -INFINITY, s, n);
    e.hi = syn_at(q.wmax, q.wmax_rs, q.wmax_cs, has_max ? wmax : INFINITY, s, n);
    return e;
}

// learning.py:87-104 / MCC_learning.py:86-110: w *= decay; w.clamp_(wmin, wmax) == min(max(w, lo), hi), a NaN weight stays NaN.
__host__ __device__ __forceinline__ float syn_finish(float w, float decay, float lo, float hi) {
    w = w * decay;
    if (w < lo) w = lo;
    if (w > hi) w = hi;
    return w;
}

// PostPre (learning.py:398-418): `pre` = sum_b s_src * (x_tgt * nu0), `post` = sum_b x_src * (s_tgt * nu1) -- the rates are already
// inside the sums.  use_dt: MCC_learning.py:238, :262.
__host__ __device__ __forceinline__ float syn_postpre(float w, bool any0, float pre, bool any1, float post, int use_dt, float dt) {
    if (any0) { if (use_dt) pre = pre * dt; w = w - pre; }
    if (any1) { if (use_dt) post = post * dt; w = w + post; }
    return w;
}

// Hebbian (learning.py:1127, :1133): both statements always run.
__host__ __device__ __forceinline__ float syn_hebbian(float w, float u1, float u2, float nu0, float nu1) {
    w = w + nu0 * u1;
    w = w + nu1 * u2;
    return w;
}

// WeightDependentPostPre (learning.py:639-651): update = 0; update -= nu0 * U1 * (w - wmin); update += nu1 * U2 * (wmax - w).
__host__ __device__ __forceinline__ float syn_wdpostpre(float w, bool any0, float u1, bool any1, float u2, float nu0, float nu1, float lo,
                                                        float hi) {
    float upd = 0.f;
    bool have = false;
    if (any0) { upd = 0.0f - (nu0 * u1) * (w - lo); have = true; }
    if (any1) { const float y = (nu1 * u2) * (hi - w); upd = have ? upd + y : y; have = true; }
    return have ? w + upd : w;
}

// MSTDP (learning.py:1561): w += nu[0] * update.
__host__ __device__ __forceinline__ float syn_mstdp(float w, float u, float nu0) { return w + nu0 * u; }

// MSTDPET (learning.py:2229-2236): the trace takes the point eligibility `el`, then w += ((nu0 * dt) * reward) * trace.
__host__ __device__ __forceinline__ float syn_mstdpet(float w, float *e_trace, float el, float decay_e, float tc_e, float nu0, float dt,
                                                      float reward) {
    float et = *e_trace * decay_e;
    et = et + el / tc_e;
    *e_trace = et;
    return w + ((nu0 * dt) * reward) * et;
}

// normalize with a tensor norm (topology.py:390-392 / topology_features.py:262-266): zero sums become 1, then norm / colsum -- one
// IEEE division, where a python-float norm is ATen's reciprocal-then-multiply (snn_normalize).
__host__ __device__ __forceinline__ float syn_norm_scale(float norm, float colsum) {
    if (colsum == 0.f) colsum = 1.0f;
    return norm / colsum;
}

// The stride pairs the *_pv entry points accept for an [Nin, N] weight matrix -- those of the five shapes that broadcast against it:
// one element (0, 0), [N] / [1, N] (0, 1), [S, 1] (1, 0), [S, N] (N, 1).  (A size-1 axis always has stride 0.)
inline bool syn_stride_ok(const float *p, int rs, int cs, int N) {
    return !p || (rs == 0 && (cs == 0 || cs == 1)) || (rs == 1 && cs == 0) || (rs == N && cs == 1);
}
inline bool syn_any(const snn_synparams *q) { return q && (q->nu0 || q->nu1 || q->wmin || q->wmax); }
inline bool syn_valid(const snn_synparams *q, int N) {
    return !q || (syn_stride_ok(q->nu0, q->nu0_rs, q->nu0_cs, N) && syn_stride_ok(q->nu1, q->nu1_rs, q->nu1_cs, N) &&
                  syn_stride_ok(q->wmin, q->wmin_rs, q->wmin_cs, N) && syn_stride_ok(q->wmax, q->wmax_rs, q->wmax_cs, N));
}

}  // namespace snn
