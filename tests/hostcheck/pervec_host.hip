// Host-side check of the step kernels' per-neuron instances (bindsnet_amd/csrc/snn_ops.hip k_input_pv / k_lif_pv / k_dc_membrane<true> /
// k_dc_arbitrate<true>, csrc/snn_nodes.hip k_node<KIND, true> / k_izh<true>): the __host__ __device__ text of csrc/snn_common.hpp --
// row_of<true> loading neuron j's row of the snn_pervec vectors, and the update functions that take the per-neuron values -- is run
// HERE on the CPU, sample by sample and neuron by neuron as the kernels' threads run it, one timestep per call;
// tests/test_pervec_hostcheck.py supplies the currents (and the one_spike draws) and compares with the reference fixtures.
// Compiled by hipcc like the kernels (same front end, -ffp-contract=off); no device code is executed.  Test infrastructure only.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_order.hpp"
#include "../../bindsnet_amd/csrc/snn_common.hpp"

using namespace snn;

// One step of k_lif_pv (kind 4) or k_node<KIND, true> (kind 0 McCullochPitts, 1 IFNodes, 2 BoostedLIFNodes, 3 CurrentLIFNodes) on a
// [B, N] layer: the sample is the outer index, neuron j indexes the vectors.  cur is masked where the kernel masks its input.
extern "C" void hostcheck_pv_step(int kind, float *v, float *refrac, float *aux, uint8_t *s, float *x, float *cur, int B, int N,
                                  const snn_lif_params *pp, float aux_decay, const snn_pervec *pv) {
    const snn_lif_params p = *pp;
    for (int b = 0; b < B; ++b)
        for (long j = 0; j < N; ++j) {
            const size_t k = (size_t)b * N + j;
            const node_row r = row_of<true>(p, aux_decay, *pv, j);
            float vv = v[k], c = cur[k];
            uint8_t sp;
            if (kind == 0) sp = mcp_update(vv, c, r.thresh);
            else {
                float rc = refrac[k];
                if (kind == 1) sp = if_update(vv, rc, c, p, r.thresh);
                else if (kind == 2 || kind == 4) {
                    if (rc > 0.f) { c = 0.f; cur[k] = 0.f; }
                    sp = kind == 2 ? boosted_update(vv, rc, c, p, r.thresh, r.decay) : lif_update(vv, rc, c, p, r.thresh, r.decay);
                } else {
                    float ii = aux[k];
                    sp = clif_update(vv, rc, ii, c, r.i_decay, p, r.thresh, r.decay);
                    aux[k] = ii;
                }
                refrac[k] = rc;
            }
            v[k] = vv; s[k] = sp;
            if (p.traces) x[k] = trace_next(x[k], sp, r.trace_decay, r.trace_scale, p.traces_additive);
        }
}

// k_dc_membrane<true>: thread <-> neuron j, the batch inside; s receives the crossings.
extern "C" void hostcheck_pv_dc_membrane(float *v, float *refrac, uint8_t *s, float *theta, const float *cur, int B, int N,
                                         const snn_dc_params *pp, const snn_pervec *pv) {
    const snn_dc_params p = *pp;
    for (int j = 0; j < N; ++j) {
        const node_row r = row_of<true>(p, 0.f, *pv, j);
        const float th0 = dc_theta_decayed(theta[j], p.learning, r.theta_decay);
        const float thr = r.thresh + th0;
        int cnt = 0;
        for (int b = 0; b < B; ++b) {
            const size_t k = (size_t)b * N + j;
            float vv = v[k], rc = refrac[k];
            const uint8_t sp = dc_update(vv, rc, cur[k], thr, p.lif, r.decay);
            v[k] = vv; refrac[k] = rc; s[k] = sp;
            cnt += sp;
        }
        theta[j] = dc_theta_bumped(th0, p.learning, r.theta_plus, cnt);
    }
}

// The trace loop of k_dc_arbitrate<true> and of k_input_pv: x after the final spikes s.
extern "C" void hostcheck_pv_trace(const uint8_t *s, float *x, int B, int N, const snn_lif_params *pp, const snn_pervec *pv) {
    const snn_lif_params p = *pp;
    for (int b = 0; b < B; ++b)
        for (long j = 0; j < N; ++j) {
            const size_t k = (size_t)b * N + j;
            const node_row r = row_of<true>(p, 0.f, *pv, j);
            x[k] = trace_next(x[k], s[k], r.trace_decay, r.trace_scale, p.traces_additive);
        }
}

// One step of k_izh<true>: per sample the entry spikes are staged as a list before any new spike is stored.
extern "C" void hostcheck_pv_izh(float *v, float *u, uint8_t *s, float *x, float *cur, const float *a, const float *b, const float *c,
                                 const float *d, const float *St, int B, int N, const snn_lif_params *pp, const snn_pervec *pv) {
    const snn_lif_params p = *pp;
    for (int smp = 0; smp < B; ++smp) {
        const size_t base = (size_t)smp * N;
        std::vector<int> list;
        std::vector<uint8_t> entry(s + base, s + base + N);
        for (int i = 0; i < N; ++i) if (entry[i]) list.push_back(i);
        for (int j = 0; j < N; ++j) {
            const float lat = inner_sum8_terms([&](int r) { return St[(size_t)list[r] * N + j]; }, (int)list.size());
            const float I = cur[base + j] + lat;
            cur[base + j] = I;
            float vv = v[base + j], uu = u[base + j];
            const node_row r = row_of<true>(p, 0.f, *pv, j);
            const uint8_t sp = izh_update(vv, uu, entry[j], I, a[j], b[j], c[j], d[j], p, r.thresh);
            v[base + j] = vv; u[base + j] = uu; s[base + j] = sp;
            if (p.traces) x[base + j] = trace_next(x[base + j], sp, r.trace_decay, r.trace_scale, p.traces_additive);
        }
    }
}
