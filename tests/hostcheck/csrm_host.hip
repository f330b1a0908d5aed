// Host-side check of bindsnet_amd/csrc/snn_csrm.hpp: the __host__ __device__ bodies of snn_prop_window_f32 and snn_csrm_step are
// run HERE on the CPU (compiled by hipcc like the kernels, no device code is executed), driven as k_prop_window / k_csrm_step drive
// them: per (sample, slot) the spiking sources are compacted chunk by chunk of 256 into an ascending list that every column then
// walks; per neuron the batch is looped with the shared theta around it.  Test infrastructure only (tests/test_csrm_hostcheck.py);
// not part of libsnnhip.
#include <stdint.h>
#include "../../bindsnet_amd/csrc/snn_common.hpp"
#include "../../bindsnet_amd/csrc/snn_csrm.hpp"

extern "C" int hostcheck_prop_window(const float *W, const float *bias, uint8_t *ring, int head, const uint8_t *s, float *out, int B,
                                     int Wn, int Nin, int N, int accumulate) {
    if (!W || !ring || !s || !out || B <= 0 || Wn <= 0 || Nin <= 0 || N <= 0 || head < 0 || head >= Wn) return -1;
    int list[256];
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < Wn; ++i) {
            const bool newest = i == Wn - 1;
            const uint8_t *src = newest ? s + (size_t)b * Nin : ring + ((size_t)b * Wn + snn::csrm_ring_slot(head, i, Wn)) * Nin;
            for (int tile = 0; tile < N; tile += 256)
                for (int j = tile; j < N && j < tile + 256; ++j) {
                    float acc = 0.0f;
                    for (int base = 0; base < Nin; base += 256) {
                        int k = 0;
                        for (int idx = base; idx < Nin && idx < base + 256; ++idx) if (src[idx]) list[k++] = idx;
                        acc = snn::csrm_gather(acc, W, list, k, N, j);
                    }
                    snn::csrm_store(out + ((size_t)b * Wn + i) * N + j, acc, bias, j, accumulate);
                }
        }
    for (int b = 0; b < B; ++b)                            // the push, behind every read of the older slots
        for (int idx = 0; idx < Nin; ++idx) ring[((size_t)b * Wn + head) * Nin + idx] = s[(size_t)b * Nin + idx] ? 1 : 0;
    return 0;
}

extern "C" int hostcheck_csrm_step(float *v, uint8_t *s, float *x, float *theta, const float *xwin, float *last, const float *resK,
                                   int Wres, const float *refK, int Wref, int B, int N, const snn_dc_params *p, const snn_pervec *vecs,
                                   float *raster_v) {
    if (!v || !s || !theta || !xwin || !last || !resK || !refK || !p || B <= 0 || N <= 0 || Wres <= 0 || Wref <= 0) return -1;
    snn_pervec pv = {};
    if (vecs) pv = *vecs;
    for (int j = 0; j < N; ++j) {
        const snn::node_row r = vecs ? snn::row_of<true>(*p, 0.f, pv, j) : snn::row_of<false>(*p, 0.f, pv, j);
        const float th0 = snn::dc_theta_decayed(theta[j], p->learning, r.theta_decay);
        const float thr = r.thresh + th0;
        int cnt = 0;
        for (int b = 0; b < B; ++b) {
            const size_t k = (size_t)b * N + j;
            float vv = v[k];
            const uint8_t sp = snn::csrm_update(vv, xwin + (size_t)b * Wres * N + j, last + (size_t)b * Wref * N + j, (size_t)N, resK, Wres,
                                                refK, Wref, thr, r.decay, p->lif);
            v[k] = vv; s[k] = sp;
            cnt += sp;
            if (p->lif.traces) x[k] = snn::trace_next(x[k], sp, r.trace_decay, r.trace_scale, p->lif.traces_additive);
            if (raster_v) raster_v[k] = vv;
        }
        theta[j] = snn::dc_theta_bumped(th0, p->learning, r.theta_plus, cnt);
    }
    return 0;
}
