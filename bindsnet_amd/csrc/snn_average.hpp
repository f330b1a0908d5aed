// snn_average.hpp -- per-element bodies of the time-averaged (`average_update` / `continues_update`) forms of the three
// MulticompartmentConnection rules (bindsnet/learning/MCC_learning.py:211-222, :237-289, :457-466, :518-535, :641-649, :696-713).
//
// A rule with average_update = K does not add a timestep's update to the weights; it stores it in slot (i0 + t) mod K of a ring of K
// weight-shaped slots and, when due, applies torch.mean(ring, dim=0): ATen's sum(dim=0) over the contiguous [K, E] ring -- the very
// reduction the rules already restate for the batch (batch_sum, snn_order.hpp), here with K terms -- followed by ONE true division by K.
// "Due": every step with continues_update, otherwise the step in which the ring index wraps to 0.  The rule's decay and clamp run every
// step.  Every weight element is independent of every other one, so one thread carries an element through the whole step.
// __host__ __device__: tests/hostcheck/average_host.hip runs these bodies on the CPU against torch (tests/test_mcc_average_hostcheck.py).
// Built with -ffp-contract=off: every operation below rounds once.
#pragma once
#include <stdint.h>
#include "snn_order.hpp"

namespace snn {

constexpr int kAvgMaxTerms = 256;      // the largest average_update (ring slots) and batch size the entry points take

struct AvgRing {
    float *buf;     // [K, E], contiguous
    int K;
    int slot;       // the slot this step's value goes to
    int due;        // apply the mean of the ring in this step
};

// The ring index at the start of a step and whether the mean is due in it (MCC_learning.py:242-253).
__host__ __device__ inline AvgRing avg_ring(float *buf, int K, int idx, int continuous) {
    AvgRing r;
    r.buf = buf; r.K = K; r.slot = idx;
    r.due = (continuous || idx + 1 == K) ? 1 : 0;
    return r;
}

// Element e's value of this step goes into its slot -- zeros included: what stands there is K steps old --; when due, *mean receives
// torch.mean(ring, dim=0)[e].
__host__ __device__ inline bool avg_push(const AvgRing &r, float val, long e, long E, float *mean) {
    r.buf[(long)r.slot * E + e] = val;
    if (!r.due) return false;
    const float *col = r.buf + e;
    const float s = batch_sum([col, E](int k) { return col[(long)k * E]; }, r.K, e, E);
    *mean = s / (float)r.K;
    return true;
}

struct AvgBounds { float decay; int has_min; float wmin; int has_max; float wmax; };

// MCC_learning.py:86-110: what every update ends with.
__host__ __device__ inline float avg_finish(float w, const AvgBounds &b) {
    w = w * b.decay;
    if (b.has_min && w < b.wmin) w = b.wmin;
    if (b.has_max && w > b.wmax) w = b.wmax;
    return w;
}

// ---- PostPre (MCC_learning.py:224-302) ------------------------------------------------------------------------------------------
struct AvgPostPre {
    const uint8_t *s_src; const float *x_src; const uint8_t *s_tgt; const float *x_tgt;     // [B, Nin] / [B, N]
    int B, Nin, N;
    float nu0, nu1, dt;
    int squeeze;                 // reduction = torch.squeeze (batch 1): the product itself, no sum
    AvgBounds fin;
    AvgRing pre, post;           // a term whose rate is 0 does not run at all: its ring and index stand still
};

// R: the batch reduction whose result goes into the ring slot (snn_order.hpp batch_sum<R>; SUM is the function as it was); the ring's own mean stays.
template <int R = kReduceSum>
__host__ __device__ inline void avg_postpre_elem(float *W, const AvgPostPre &a, long e) {
    const long E = (long)a.Nin * a.N;
    const int i = (int)(e / a.N), j = (int)(e - (long)i * a.N);
    float w = W[e], m;
    if (a.nu0 != 0.f) {          // reduction(bmm(s_src, x_tgt * nu0), dim=0)
        auto term = [&a, i, j](int b) { return (float)a.s_src[(long)b * a.Nin + i] * (a.x_tgt[(long)b * a.N + j] * a.nu0); };
        const float v = a.squeeze ? term(0) : batch_sum<R>(term, a.B, e, E);
        if (avg_push(a.pre, v, e, E, &m)) w = w - m * a.dt;
    }
    if (a.nu1 != 0.f) {          // reduction(bmm(x_src, s_tgt * nu1), dim=0)
        auto term = [&a, i, j](int b) { return a.x_src[(long)b * a.Nin + i] * ((float)a.s_tgt[(long)b * a.N + j] * a.nu1); };
        const float v = a.squeeze ? term(0) : batch_sum<R>(term, a.B, e, E);
        if (avg_push(a.post, v, e, E, &m)) w = w + m * a.dt;
    }
    W[e] = avg_finish(w, a.fin);
}

// ---- MSTDP (MCC_learning.py:468-548) --------------------------------------------------------------------------------------------
// The eligibility of the previous step is kept as its factors, as in snn_mstdp_step: elig[b] = p_plus[b] (x) s_tgt_prev[b] +
// s_src_prev[b] (x) p_minus[b].  The factors advance behind this pass (every element reads them).
struct AvgMstdp {
    const float *p_plus, *p_minus; const uint8_t *s_src_prev, *s_tgt_prev;                  // [B, Nin] / [B, N]
    int B, Nin, N;
    float reward; const float *reward_vec;
    float nu0;
    int squeeze;
    AvgBounds fin;
    AvgRing ring;
};

template <int R = kReduceSum>
__host__ __device__ inline void avg_mstdp_elem(float *W, const AvgMstdp &a, long e) {
    const long E = (long)a.Nin * a.N;
    const int i = (int)(e / a.N), j = (int)(e - (long)i * a.N);
    auto term = [&a, i, j](int b) {
        const float e1 = a.p_plus[(long)b * a.Nin + i] * (float)a.s_tgt_prev[(long)b * a.N + j];
        const float e2 = (float)a.s_src_prev[(long)b * a.Nin + i] * a.p_minus[(long)b * a.N + j];
        const float el = e1 + e2;
        return (a.reward_vec ? a.reward_vec[b] : a.reward) * el;       // reward * eligibility
    };
    const float v = a.squeeze ? term(0) : batch_sum<R>(term, a.B, e, E);
    float w = W[e], m;
    if (avg_push(a.ring, v, e, E, &m)) w = w + a.nu0 * m;              // :527-530
    W[e] = avg_finish(w, a.fin);
}

// ---- MSTDPET (MCC_learning.py:652-733, batch 1) ---------------------------------------------------------------------------------
struct AvgMstdpet {
    float *e_trace;                                                                          // [Nin, N], in/out
    const float *p_plus, *p_minus; const uint8_t *s_src_prev, *s_tgt_prev;                  // [Nin] / [N]
    int Nin, N;
    float scale;                 // (nu0 * dt) * reward
    float decay_e, tc_e;
    AvgBounds fin;
    AvgRing ring;
};

__host__ __device__ inline void avg_mstdpet_elem(float *W, const AvgMstdpet &a, long e) {
    const long E = (long)a.Nin * a.N;
    const int i = (int)(e / a.N), j = (int)(e - (long)i * a.N);
    const float el = a.p_plus[i] * (float)a.s_tgt_prev[j] + (float)a.s_src_prev[i] * a.p_minus[j];
    float et = a.e_trace[e] * a.decay_e;               // :688-690
    et = et + el / a.tc_e;                             // :691
    a.e_trace[e] = et;
    float w = W[e], m;
    if (avg_push(a.ring, a.scale * et, e, E, &m)) w = w + m;          // :697-708
    W[e] = avg_finish(w, a.fin);
}

// P+ / P- and the previous-step spikes of the reward rules (MCC_learning.py:538-541 / :716-719), element k of n_src + n_tgt.
__host__ __device__ inline void avg_trace_elem(float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                                               const uint8_t *s_tgt, long n_src, long k, float a_plus, float a_minus, float d_plus,
                                               float d_minus) {
    if (k < n_src) {
        const uint8_t sv = s_src[k];
        const float p = p_plus[k] * d_plus;
        p_plus[k] = p + a_plus * (float)sv;
        s_src_prev[k] = sv;
    } else {
        const long q = k - n_src;
        const uint8_t sv = s_tgt[q];
        const float p = p_minus[q] * d_minus;
        p_minus[q] = p + a_minus * (float)sv;
        s_tgt_prev[q] = sv;
    }
}

}  // namespace snn
