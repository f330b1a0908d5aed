// The per-synapse update bodies of csrc/snn_synparams.hpp on the HOST: compiled with hipcc (no GPU needed) and driven element by
// element, as the threads of k_plasticity_pv / k_mstdpet_pv / k_colsum_nv do -- same accessors, same bodies, the batch sums through
// the same ATen-ordered accumulator (snn_order.hpp).  tests/test_synparams_hostcheck.py compares against reference fixtures and torch.
#include <stdint.h>
#include "../../bindsnet_amd/csrc/snn_order.hpp"
#include "../../bindsnet_amd/csrc/snn_synparams.hpp"

using namespace snn;

// mode 0: PostPre (x_tgt * nu0 and s_tgt * nu1 inside the sums), 1: MSTDP's weight step (x_src = p_plus, x_tgt = p_minus, s_* the previous
// step's spikes), 2: Hebbian, 3: WeightDependentPostPre.  nu0 / nu1: the scalar rate, or for a rate given in `q` 1 / 0 = "any entry non-zero".
extern "C" int hostcheck_syn_update(int mode, float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt,
                                    int B, int Nin, int N, float nu0, float nu1, int use_dt, float dt, float decay, int has_min, float wmin,
                                    int has_max, float wmax, const snn_synparams *q, float reward, const float *reward_vec) {
    if (!syn_valid(q, N)) return -1;
    if (mode == 0 && ((q->nu0 && q->nu0_rs) || (q->nu1 && q->nu1_rs))) return -1;
    const float g0 = q->nu0 ? (q->nu0_any ? 1.f : 0.f) : nu0, g1 = q->nu1 ? (q->nu1_any ? 1.f : 0.f) : nu1;
    const long E = (long)Nin * N, Emain = (E / 32) * 32;
    for (int i = 0; i < Nin; ++i)
        for (int j = 0; j < N; ++j) {
            const long e = (long)i * N + j;
            const bool tail = e >= Emain;
            const SynElem c = syn_elem(*q, nu0, nu1, has_min, wmin, has_max, wmax, i, j);
            float w = W[e];
            OuterSum a1, a2;
            a1.init(tail); a2.init(tail);
            if (mode == 0) {
                const float n0 = syn_at(q->nu0, 0, q->nu0_cs, nu0, 0, j);
                for (int b = 0; b < B; ++b) {
                    if (s_src[(long)b * Nin + i]) a1.add(b, (float)s_src[(long)b * Nin + i] * (x_tgt[(long)b * N + j] * n0), B);
                    if (s_tgt[(long)b * N + j]) a2.add(b, x_src[(long)b * Nin + i] * ((float)s_tgt[(long)b * N + j] * c.nu1), B);
                }
                const float pre = g0 != 0.f ? a1.finish(B) : 0.f, post = g1 != 0.f ? a2.finish(B) : 0.f;
                w = syn_postpre(w, g0 != 0.f, pre, false, 0.f, use_dt, dt);
                w = syn_postpre(w, false, 0.f, g1 != 0.f, post, use_dt, dt);
            } else if (mode == 1) {
                for (int b = 0; b < B; ++b) {
                    if (!s_src[(long)b * Nin + i] && !s_tgt[(long)b * N + j]) continue;
                    const float e1 = x_src[(long)b * Nin + i] * (float)s_tgt[(long)b * N + j];
                    const float e2 = (float)s_src[(long)b * Nin + i] * x_tgt[(long)b * N + j];
                    const float el = e1 + e2;
                    a1.add(b, (reward_vec ? reward_vec[b] : reward) * el, B);
                }
                w = syn_mstdp(w, a1.finish(B), c.nu0);
            } else {
                for (int b = 0; b < B; ++b) {
                    if (s_src[(long)b * Nin + i]) a1.add(b, (float)s_src[(long)b * Nin + i] * x_tgt[(long)b * N + j], B);
                    if (s_tgt[(long)b * N + j]) a2.add(b, x_src[(long)b * Nin + i] * (float)s_tgt[(long)b * N + j], B);
                }
                const float u1 = a1.finish(B), u2 = a2.finish(B);
                w = mode == 2 ? syn_hebbian(w, u1, u2, c.nu0, c.nu1) : syn_wdpostpre(w, g0 != 0.f, u1, g1 != 0.f, u2, c.nu0, c.nu1, c.lo, c.hi);
            }
            W[e] = syn_finish(w, decay, c.lo, c.hi);
        }
    return 0;
}

extern "C" int hostcheck_syn_mstdpet(float *W, float *e_trace, const float *p_plus, const float *p_minus, const uint8_t *s_src_prev,
                                     const uint8_t *s_tgt_prev, int Nin, int N, float reward, float nu0, float dt, float decay_e, float tc_e,
                                     float wdecay, int has_min, float wmin, int has_max, float wmax, const snn_synparams *q) {
    if (!syn_valid(q, N)) return -1;
    for (int i = 0; i < Nin; ++i)
        for (int j = 0; j < N; ++j) {
            const long e = (long)i * N + j;
            const SynElem c = syn_elem(*q, nu0, 0.f, has_min, wmin, has_max, wmax, i, j);
            const float el = p_plus[i] * (float)s_tgt_prev[j] + (float)s_src_prev[i] * p_minus[j];
            const float w = syn_mstdpet(W[e], &e_trace[e], el, decay_e, tc_e, c.nu0, dt, reward);
            W[e] = syn_finish(w, wdecay, c.lo, c.hi);
        }
    return 0;
}

// scale[n] = norm[n] / colsum[n] (zero sums -> 1), then W *= scale per column
extern "C" int hostcheck_syn_normalize(float *W, const float *colsum, const float *norm, int Nin, int N) {
    for (int i = 0; i < Nin; ++i)
        for (int j = 0; j < N; ++j) W[(long)i * N + j] = W[(long)i * N + j] * syn_norm_scale(norm[j], colsum[j]);
    return 0;
}
