// Host-side check of the node step kernels of bindsnet_amd/csrc/snn_nodes.hip: the __host__ __device__ update bodies of
// csrc/snn_common.hpp (mcp_update, if_update, boosted_update, clif_update, izh_update, trace_next) and the lateral-sum accumulator
// (csrc/snn_order.hpp inner_sum8_terms over the ascending list of spiking neurons) are run HERE on the CPU, element by element
// and term by term as a kernel thread runs them, and compared with the reference fixtures / with torch by
// tests/test_nodes_hostcheck.py.  Compiled by hipcc like the kernels (same front end, -ffp-contract=off); no device code is
// executed.  Test infrastructure only; not part of libsnnhip.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_order.hpp"
#include "../../bindsnet_amd/csrc/snn_common.hpp"

using namespace snn;

// k_node<KIND>'s thread per element, T steps: kind 0 McCullochPitts, 1 IFNodes, 2 BoostedLIFNodes, 3 CurrentLIFNodes.
// cur [T, n] is written where the kernel writes its input (BoostedLIFNodes' mask); raster [T, n], vrec [T, n].
extern "C" void hostcheck_node_run(int kind, float *v, float *refrac, float *aux, uint8_t *s, float *x, float *cur, int T, long n,
                                   const snn_lif_params *pp, float aux_decay, uint8_t *raster, float *vrec) {
    const snn_lif_params p = *pp;
    for (int t = 0; t < T; ++t)
        for (long k = 0; k < n; ++k) {
            float *I = cur + (size_t)t * n;
            float vv = v[k], c = I[k];
            uint8_t sp;
            if (kind == 0) sp = mcp_update(vv, c, p);
            else {
                float rc = refrac[k];
                if (kind == 1) sp = if_update(vv, rc, c, p);
                else if (kind == 2) {
                    if (rc > 0.f) { c = 0.f; I[k] = 0.f; }
                    sp = boosted_update(vv, rc, c, p);
                } else {
                    float ii = aux[k];
                    sp = clif_update(vv, rc, ii, c, aux_decay, p);
                    aux[k] = ii;
                }
                refrac[k] = rc;
            }
            v[k] = vv; s[k] = sp;
            if (p.traces) x[k] = trace_next(x[k], sp, p.trace_decay, p.trace_scale, p.traces_additive);
            raster[(size_t)t * n + k] = sp;
            vrec[(size_t)t * n + k] = vv;
        }
}

// k_izh's thread j of sample b: the lateral sum over the ascending list of the sample's entry spikes, term r = St[list[r], j].
static float lateral(const float *St, const std::vector<int> &list, int N, int j) {
    return inner_sum8_terms([&](int r) { return St[(size_t)list[r] * N + j]; }, (int)list.size());
}

// out[j] = the kernel's sum for the neurons selected by mask [N] (what torch computes as S[:, mask].sum(dim=1)).
extern "C" void hostcheck_lateral(const float *St, const uint8_t *mask, int N, float *out) {
    std::vector<int> list;
    for (int i = 0; i < N; ++i) if (mask[i]) list.push_back(i);
    for (int j = 0; j < N; ++j) out[j] = lateral(St, list, N, j);
}

// k_izh, T steps: per sample the entry spikes are staged as a list before any new spike is stored.
extern "C" void hostcheck_izh_run(float *v, float *u, uint8_t *s, float *x, float *cur, const float *a, const float *b, const float *c,
                                  const float *d, const float *St, int B, int N, int T, const snn_lif_params *pp, uint8_t *raster,
                                  float *vrec) {
    const snn_lif_params p = *pp;
    for (int t = 0; t < T; ++t)
        for (int smp = 0; smp < B; ++smp) {
            const size_t base = (size_t)smp * N, off = ((size_t)t * B + smp) * N;
            std::vector<int> list;
            std::vector<uint8_t> entry(s + base, s + base + N);
            for (int i = 0; i < N; ++i) if (entry[i]) list.push_back(i);
            for (int j = 0; j < N; ++j) {
                const float I = cur[off + j] + lateral(St, list, N, j);
                cur[off + j] = I;
                float vv = v[base + j], uu = u[base + j];
                const uint8_t sp = izh_update(vv, uu, entry[j], I, a[j], b[j], c[j], d[j], p);
                v[base + j] = vv; u[base + j] = uu; s[base + j] = sp;
                if (p.traces) x[base + j] = trace_next(x[base + j], sp, p.trace_decay, p.trace_scale, p.traces_additive);
                raster[off + j] = sp;
                vrec[off + j] = vv;
            }
        }
}
