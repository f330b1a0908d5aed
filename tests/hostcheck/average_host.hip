// Host-side check of bindsnet_amd/csrc/snn_average.hpp: the __host__ __device__ bodies of the time-averaged MCC rules are run HERE on
// the CPU (compiled by hipcc like the kernels, no device code is executed), element by element as the threads of k_avg_postpre /
// k_avg_mstdp / k_avg_mstdpet run them, the factors of the reward rules behind the weight pass as k_avg_traces does.  Test
// infrastructure only (tests/test_mcc_average_hostcheck.py); not part of libsnnhip.
#include <stdint.h>
#include "../../bindsnet_amd/csrc/snn_average.hpp"

using namespace snn;

// out [E] = torch.mean(ring [K, E], dim=0) as avg_push forms it (slot 0 rewritten with its own value, the mean due)
extern "C" int hostcheck_avg_mean(float *ring, int K, long E, float *out) {
    if (K < 1 || K > kAvgMaxTerms || E < 1) return -1;
    const AvgRing r = avg_ring(ring, K, 0, 1);
    for (long e = 0; e < E; ++e)
        if (!avg_push(r, ring[e], e, E, &out[e])) return -2;
    return 0;
}

extern "C" int hostcheck_avg_postpre(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                                     int Nin, int N, float nu0, float nu1, float dt, float decay, int has_min, float wmin, int has_max,
                                     float wmax, int squeeze, float *ring_pre, float *ring_post, int K, int continuous, int idx_pre,
                                     int idx_post) {
    if (K < 1 || K > kAvgMaxTerms || idx_pre < 0 || idx_pre >= K || idx_post < 0 || idx_post >= K) return -1;
    AvgPostPre a;
    a.s_src = s_src; a.x_src = x_src; a.s_tgt = s_tgt; a.x_tgt = x_tgt;
    a.B = B; a.Nin = Nin; a.N = N;
    a.nu0 = nu0; a.nu1 = nu1; a.dt = dt; a.squeeze = squeeze;
    a.fin = AvgBounds{decay, has_min, wmin, has_max, wmax};
    a.pre = avg_ring(ring_pre, K, idx_pre, continuous);
    a.post = avg_ring(ring_post, K, idx_post, continuous);
    for (long e = 0; e < (long)Nin * N; ++e) avg_postpre_elem(W, a, e);
    return 0;
}

static void traces(float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src, const uint8_t *s_tgt,
                   long n_src, long n_tgt, float a_plus, float a_minus, float d_plus, float d_minus) {
    for (long k = 0; k < n_src + n_tgt; ++k)
        avg_trace_elem(p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, n_src, k, a_plus, a_minus, d_plus, d_minus);
}

extern "C" int hostcheck_avg_mstdp(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                                   const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0,
                                   float a_plus, float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin,
                                   int has_max, float wmax, int squeeze, float *ring, int K, int continuous, int idx) {
    if (K < 1 || K > kAvgMaxTerms || idx < 0 || idx >= K) return -1;
    AvgMstdp a;
    a.p_plus = p_plus; a.p_minus = p_minus; a.s_src_prev = s_src_prev; a.s_tgt_prev = s_tgt_prev;
    a.B = B; a.Nin = Nin; a.N = N;
    a.reward = reward; a.reward_vec = reward_vec; a.nu0 = nu0; a.squeeze = squeeze;
    a.fin = AvgBounds{wdecay, has_min, wmin, has_max, wmax};
    a.ring = avg_ring(ring, K, idx, continuous);
    for (long e = 0; e < (long)Nin * N; ++e) avg_mstdp_elem(W, a, e);
    traces(p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, (long)B * Nin, (long)B * N, a_plus, a_minus, decay_plus, decay_minus);
    return 0;
}

extern "C" int hostcheck_avg_mstdpet(float *W, float *e_trace, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev,
                                     const uint8_t *s_src, const uint8_t *s_tgt, int Nin, int N, float reward, float nu0, float dt,
                                     float a_plus, float a_minus, float decay_plus, float decay_minus, float decay_e, float tc_e,
                                     float wdecay, int has_min, float wmin, int has_max, float wmax, float *ring, int K, int continuous,
                                     int idx) {
    if (K < 1 || K > kAvgMaxTerms || idx < 0 || idx >= K) return -1;
    AvgMstdpet a;
    a.e_trace = e_trace; a.p_plus = p_plus; a.p_minus = p_minus; a.s_src_prev = s_src_prev; a.s_tgt_prev = s_tgt_prev;
    a.Nin = Nin; a.N = N;
    a.scale = (nu0 * dt) * reward;
    a.decay_e = decay_e; a.tc_e = tc_e;
    a.fin = AvgBounds{wdecay, has_min, wmin, has_max, wmax};
    a.ring = avg_ring(ring, K, idx, continuous);
    for (long e = 0; e < (long)Nin * N; ++e) avg_mstdpet_elem(W, a, e);
    traces(p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, (long)Nin, (long)N, a_plus, a_minus, decay_plus, decay_minus);
    return 0;
}
