// snn_common.hpp -- elementwise neuron updates shared by the per-op kernels and the fused drivers.
// Each function restates one reference forward() in its exact f32 op order (no FMA: the library is
// built with -ffp-contract=off, so every * and + below is a separately rounded instruction).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"

int snn_check_launch();            // snn_api.hip: hipGetLastError() -> SNN_* code
int snn_check(hipError_t e);
// snn_ops.hip: the event-driven dense propagation whose workgroups of a flagged tile return at once (the second launch of snn_prop_dense_auto_f32)
int snn_launch_prop_dense_flagged(const float *W, const float *bias, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate,
                                  const int *flags, hipStream_t stream);

namespace snn {

// Nodes.forward trace, bindsnet/network/nodes.py:96-103.
__host__ __device__ __forceinline__ float trace_next(float x, uint8_t s, float decay, float scale, int additive) {
    float t = x * decay;
    if (additive) t = t + scale * (float)s;
    else if (s) t = scale;
    return t;
}

// LIFNodes.forward, bindsnet/network/nodes.py:508-527.  `cur` must already be zeroed by the
// caller where rc > 0 (nodes.py:511 masks with the refractory counter BEFORE it is decremented).
// `thresh`, `decay`: this neuron's values (the scalars of `p`, or row j of per-neuron vectors: nodes.py takes either).
__host__ __device__ __forceinline__ uint8_t lif_update(float &v, float &rc, float cur, const snn_lif_params &p, float thresh,
                                                       float decay) {
    float vv = v - p.rest;              // :508  decay * (v - rest) + rest, three roundings
    vv = decay * vv;
    vv = vv + p.rest;
    rc = rc - p.dt;                     // :514
    vv = vv + cur;                      // :516
    const uint8_t sp = vv >= thresh;    // :519
    if (sp) { rc = p.refrac; vv = p.reset; }                 // :522-523
    if (p.has_lbound && vv < p.lbound) vv = p.lbound;        // :526-527
    v = vv;
    return sp;
}

__host__ __device__ __forceinline__ uint8_t lif_update(float &v, float &rc, float cur, const snn_lif_params &p) {
    return lif_update(v, rc, cur, p, p.thresh, p.decay);
}

// DiehlAndCookNodes.forward membrane part, bindsnet/network/nodes.py:1077-1092 (+ :1108-1109).
// thr = thresh + theta[j] (already decayed), computed once per neuron by the caller.
// `decay`: this neuron's value, as in lif_update.
__host__ __device__ __forceinline__ uint8_t dc_update(float &v, float &rc, float cur, float thr, const snn_lif_params &p,
                                                      float decay) {
    float vv = v - p.rest;              // :1077
    vv = decay * vv;
    vv = vv + p.rest;
    const float gate = (rc <= 0.f) ? 1.0f : 0.0f;            // :1082 (refrac_count <= 0).float() * x
    const float gx = gate * cur;
    vv = vv + gx;
    rc = rc - p.dt;                     // :1085
    const uint8_t sp = vv >= thr;       // :1088
    if (sp) { rc = p.refrac; vv = p.reset; }                 // :1091-1092
    if (p.has_lbound && vv < p.lbound) vv = p.lbound;        // :1108-1109
    v = vv;
    return sp;
}

__host__ __device__ __forceinline__ uint8_t dc_update(float &v, float &rc, float cur, float thr, const snn_lif_params &p) {
    return dc_update(v, rc, cur, thr, p, p.decay);
}

// The adaptive threshold around dc_update, nodes.py:1078-1079 and :1093-1094: theta decays before the membrane step and grows by
// theta_plus per crossing of the batch after it, both only while learning.  `count` is exact in f32; one rounded multiply, one add.
__host__ __device__ __forceinline__ float dc_theta_decayed(float theta, int learning, float theta_decay) {
    return learning ? theta * theta_decay : theta;
}
__host__ __device__ __forceinline__ float dc_theta_bumped(float theta, int learning, float theta_plus, int count) {
    if (!learning) return theta;
    const float bump = theta_plus * (float)count;
    return theta + bump;
}

// McCullochPitts.forward, bindsnet/network/nodes.py:285-286.
__host__ __device__ __forceinline__ uint8_t mcp_update(float &v, float cur, float thresh) {
    v = cur;                            // :285 (the reference aliases; the layer keeps a copy)
    return v >= thresh;                 // :286
}
__host__ __device__ __forceinline__ uint8_t mcp_update(float &v, float cur, const snn_lif_params &p) {
    return mcp_update(v, cur, p.thresh);
}

// IFNodes.forward, bindsnet/network/nodes.py:379-393.  No decay, no rest; the gate reads rc BEFORE the decrement.
__host__ __device__ __forceinline__ uint8_t if_update(float &v, float &rc, float cur, const snn_lif_params &p, float thresh) {
    const float gate = (rc <= 0.f) ? 1.0f : 0.0f;            // :379 (refrac_count <= 0).float() * x
    const float gx = gate * cur;
    float vv = v + gx;
    rc = rc - p.dt;                     // :382
    const uint8_t sp = vv >= thresh;    // :385
    if (sp) { rc = p.refrac; vv = p.reset; }                 // :388-389
    if (p.has_lbound && vv < p.lbound) vv = p.lbound;        // :392-393
    v = vv;
    return sp;
}
__host__ __device__ __forceinline__ uint8_t if_update(float &v, float &rc, float cur, const snn_lif_params &p) {
    return if_update(v, rc, cur, p, p.thresh);
}

// BoostedLIFNodes.forward, bindsnet/network/nodes.py:629-646.  `cur` must already be zeroed by the caller where rc > 0
// (:633 masks with the counter BEFORE it is decremented).  No rest, no lbound; the reset value is the constant 0.
__host__ __device__ __forceinline__ uint8_t boosted_update(float &v, float &rc, float cur, const snn_lif_params &p, float thresh,
                                                           float decay) {
    float vv = v * decay;               // :629
    rc = rc - p.dt;                     // :636
    vv = vv + cur;                      // :639
    const uint8_t sp = vv >= thresh;    // :642
    if (sp) { rc = p.refrac; vv = 0.f; }                     // :645-646
    v = vv;
    return sp;
}
__host__ __device__ __forceinline__ uint8_t boosted_update(float &v, float &rc, float cur, const snn_lif_params &p) {
    return boosted_update(v, rc, cur, p, p.thresh, p.decay);
}

// CurrentLIFNodes.forward, bindsnet/network/nodes.py:770-789.  The gate reads rc AFTER the decrement.
__host__ __device__ __forceinline__ uint8_t clif_update(float &v, float &rc, float &i, float cur, float i_decay,
                                                        const snn_lif_params &p, float thresh, float decay) {
    float vv = v - p.rest;              // :770
    vv = decay * vv;
    vv = vv + p.rest;
    float ii = i * i_decay;             // :771
    rc = rc - p.dt;                     // :774
    ii = ii + cur;                      // :777
    const float gate = (rc <= 0.f) ? 1.0f : 0.0f;            // :778
    const float gi = gate * ii;
    vv = vv + gi;
    const uint8_t sp = vv >= thresh;    // :781
    if (sp) { rc = p.refrac; vv = p.reset; }                 // :784-785
    if (p.has_lbound && vv < p.lbound) vv = p.lbound;        // :788-789
    v = vv; i = ii;
    return sp;
}
__host__ __device__ __forceinline__ uint8_t clif_update(float &v, float &rc, float &i, float cur, float i_decay,
                                                        const snn_lif_params &p) {
    return clif_update(v, rc, i, cur, i_decay, p, p.thresh, p.decay);
}

// IzhikevichNodes.forward without its lateral sum, bindsnet/network/nodes.py:1274-1294.  s_in: last step's spike of this
// neuron; cur: the input current with the lateral sum already added (:1279).
__host__ __device__ __forceinline__ uint8_t izh_update(float &v, float &u, uint8_t s_in, float cur, float a, float b, float c,
                                                       float d, const snn_lif_params &p, float thresh) {
    float vv = v, uu = u;
    if (s_in) { vv = c; uu = uu + d; }  // :1274-1275
    const float h = p.dt * 0.5f;
    for (int half = 0; half < 2; ++half) {                   // :1285-1286, left to right
        float t = vv * vv;              // v**2
        t = 0.04f * t;
        const float t5 = 5.0f * vv;
        t = t + t5;
        t = t + 140.0f;
        t = t - uu;
        t = t + cur;
        t = h * t;
        vv = vv + t;
    }
    const float da = p.dt * a;          // :1287
    float w = b * vv;
    w = w - uu;
    w = da * w;
    uu = uu + w;
    if (p.has_lbound && vv < p.lbound) vv = p.lbound;        // :1290-1291
    v = vv; u = uu;
    return vv >= thresh;                // :1294
}
__host__ __device__ __forceinline__ uint8_t izh_update(float &v, float &u, uint8_t s_in, float cur, float a, float b, float c,
                                                       float d, const snn_lif_params &p) {
    return izh_update(v, u, s_in, cur, a, b, c, d, p, p.thresh);
}

// SRM0Nodes.forward, bindsnet/network/nodes.py:1647-1669.  `u`: this element's uniform draw (:1661 torch.rand_like, one 32-bit
// generator output: srm0_uniform).  `ex`: the exponential -- expf on the device, the host's in tests/hostcheck/srm0_host.hip;
// everything else is this text.  rho and s_prob are the layer's attributes of the same names (rho is taken BEFORE the reset).
__host__ __device__ __forceinline__ float srm0_uniform(uint32_t tempered) {
    return (float)(tempered & 0xFFFFFFu) * 5.9604644775390625e-08f;       // (r & (2^24 - 1)) * 2^-24, exact in f32
}
template <class EXP>
__host__ __device__ __forceinline__ uint8_t srm0_update(float &v, float &rc, float cur, float u, float &s_prob, float &rho,
                                                        const snn_lif_params &p, float thresh, float decay, float eps_0,
                                                        float rho_0, float d_thresh, EXP ex) {
    float vv = v - p.rest;              // :1647  decay * (v - rest) + rest, three roundings
    vv = decay * vv;
    vv = vv + p.rest;
    const float gate = (rc <= 0.f) ? 1.0f : 0.0f;            // :1650 ((refrac_count <= 0).float() * eps_0) * x
    const float ge = gate * eps_0;
    const float gx = ge * cur;
    vv = vv + gx;
    float a = vv - thresh;              // :1654 rho_0 * exp((v - thresh) / d_thresh)
    a = a / d_thresh;
    const float r = rho_0 * ex(a);
    float b = -r;                       // :1655 1.0 - exp(-rho * dt)
    b = b * p.dt;
    const float sp_ = 1.0f - ex(b);
    rho = r; s_prob = sp_;
    rc = rc - p.dt;                     // :1658
    const uint8_t sp = u < sp_;         // :1661
    if (sp) { rc = p.refrac; vv = p.reset; }                 // :1664-1665
    if (p.has_lbound && vv < p.lbound) vv = p.lbound;        // :1668-1669
    v = vv;
    return sp;
}

// Rmax._connection_update, bindsnet/learning/learning.py:2948-2958 (+ LearningRule.update :87-104), batch 1.
// rmax_term: the per-target factor s_j - p_j / (1 + (tc_c / dt) * p_j), q = tc_c / dt.  rmax_update: one synapse --
// e = e * k + term_j * x_i (k = 1 - dt / tc_e_trace), w += (nu0 * reward) * e, w *= wdecay, clamp.
struct rmax_consts { float k, q, scale; };
__host__ __device__ __forceinline__ rmax_consts rmax_constants(float reward, float nu0, float dt, float tc_c, float tc_e) {
    rmax_consts c;
    c.k = dt / tc_e;                    // :2948  1 - dt / tc_e_trace: a Python float over a 0-dim f32 tensor, evaluated in f32
    c.k = 1.0f - c.k;
    c.q = tc_c / dt;                    // :2951
    c.scale = nu0 * reward;             // :2955  (nu[0] * reward) * eligibility_trace
    return c;
}
__host__ __device__ __forceinline__ float rmax_term(uint8_t s, float p, float q) {
    float d = q * p;
    d = 1.0f + d;
    d = p / d;
    return (float)s - d;
}
__host__ __device__ __forceinline__ void rmax_update(float &w, float &e, float term, float x, float k, float scale, float wdecay,
                                                     int has_min, float wmin, int has_max, float wmax) {
    float ee = e * k;                   // :2948
    const float tx = term * x;          // :2949-2952
    ee = ee + tx;
    e = ee;
    const float up = scale * ee;        // :2955
    float ww = w + up;                  // :2958
    ww = ww * wdecay;                   // :93-94
    if (has_min && ww < wmin) ww = wmin;                     // :104
    if (has_max && ww > wmax) ww = wmax;
    w = ww;
}

// One neuron's seven parameters: the scalars of the layer's parameter block, or -- PV, the instance a launch with vectors selects --
// row j of whichever snn_pervec vectors are given.  The scalar instance reads no pointer and indexes nothing.
struct node_row { float thresh, decay, trace_decay, trace_scale, theta_decay, theta_plus, i_decay; };

template <bool PV>
__host__ __device__ __forceinline__ node_row row_of(const snn_dc_params &p, float i_decay, const snn_pervec &pv, long j) {
    node_row r = {p.lif.thresh, p.lif.decay, p.lif.trace_decay, p.lif.trace_scale, p.theta_decay, p.theta_plus, i_decay};
    if (PV) {
        if (pv.v[SNN_PV_THRESH]) r.thresh = pv.v[SNN_PV_THRESH][j];
        if (pv.v[SNN_PV_DECAY]) r.decay = pv.v[SNN_PV_DECAY][j];
        if (pv.v[SNN_PV_TRACE_DECAY]) r.trace_decay = pv.v[SNN_PV_TRACE_DECAY][j];
        if (pv.v[SNN_PV_TRACE_SCALE]) r.trace_scale = pv.v[SNN_PV_TRACE_SCALE][j];
        if (pv.v[SNN_PV_THETA_DECAY]) r.theta_decay = pv.v[SNN_PV_THETA_DECAY][j];
        if (pv.v[SNN_PV_THETA_PLUS]) r.theta_plus = pv.v[SNN_PV_THETA_PLUS][j];
        if (pv.v[SNN_PV_I_DECAY]) r.i_decay = pv.v[SNN_PV_I_DECAY][j];
    }
    return r;
}
template <bool PV>
__host__ __device__ __forceinline__ node_row row_of(const snn_lif_params &p, float i_decay, const snn_pervec &pv, long j) {
    snn_dc_params q = {};
    q.lif = p;
    return row_of<PV>(q, i_decay, pv, j);
}

// True when `pv` names a vector; `allowed`: bit q set where the layer kind reads SNN_PV_q (a vector outside it is an error).
inline bool pervec_any(const snn_pervec *pv) {
    if (pv) for (int q = 0; q < SNN_PV_COUNT; ++q) if (pv->v[q]) return true;
    return false;
}
inline bool pervec_within(const snn_pervec *pv, unsigned allowed) {
    if (pv) for (int q = 0; q < SNN_PV_COUNT; ++q) if (pv->v[q] && !((allowed >> q) & 1u)) return false;
    return true;
}
enum : unsigned { kPvTrace = 1u << SNN_PV_TRACE_DECAY | 1u << SNN_PV_TRACE_SCALE, kPvThresh = 1u << SNN_PV_THRESH,
                  kPvDecay = 1u << SNN_PV_DECAY, kPvTheta = 1u << SNN_PV_THETA_DECAY | 1u << SNN_PV_THETA_PLUS,
                  kPvIDecay = 1u << SNN_PV_I_DECAY };

}  // namespace snn
