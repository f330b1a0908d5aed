// Host-side check of bindsnet_amd/csrc/snn_real.hip: the __host__ __device__ bodies of csrc/snn_real.hpp (real_term, real_finish,
// real_trace_next, real_dense_chain, real_conv2d_chains) are run HERE on the CPU, element by element as a kernel thread runs them,
// and compared with the numpy stated order by tests/test_analog_hostcheck.py.  Compiled by hipcc like the kernels (same front
// end, -ffp-contract=off); no device code is executed.  Test infrastructure only; not part of libsnnhip.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_common.hpp"
#include "../../bindsnet_amd/csrc/snn_real.hpp"

using namespace snn;

// k_dense_real's lane per (sample tile, column): the chains of `tile` samples advance together, and a source is left out where
// every sample of the tile is zero there (the wave's ballot); tile <= 0: one chain at a time through real_dense_chain, every
// zero skipped.
extern "C" int hostcheck_dense_real(const float *W, const float *bias, const float *x, float *out, int B, int Nin, int N,
                                    int accumulate, int tile) {
    if (tile > 16) return -1;
    if (tile <= 0) {
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < N; ++j) {
                const float acc = real_dense_chain([&](int i) { return x[(size_t)b * Nin + i]; }, [&](int i) { return W[(size_t)i * N + j]; }, Nin, true);
                const size_t o = (size_t)b * N + j;
                out[o] = real_finish(acc, bias != nullptr, bias ? bias[j] : 0.0f, accumulate, accumulate ? out[o] : 0.0f);
            }
        return 0;
    }
    for (int b0 = 0; b0 < B; b0 += tile)
        for (int j = 0; j < N; ++j) {
            float acc[16];
            for (int t = 0; t < tile; ++t) acc[t] = 0.0f;
            for (int i = 0; i < Nin; ++i) {
                float xv[16];
                bool any = false;
                for (int t = 0; t < tile; ++t) { xv[t] = b0 + t < B ? x[(size_t)(b0 + t) * Nin + i] : 0.0f; any = any || xv[t] != 0.0f; }
                if (!any) continue;
                for (int t = 0; t < tile; ++t) real_term(acc[t], xv[t], W[(size_t)i * N + j]);
            }
            for (int t = 0; t < tile && b0 + t < B; ++t) {
                const size_t o = (size_t)(b0 + t) * N + j;
                out[o] = real_finish(acc[t], bias != nullptr, bias ? bias[j] : 0.0f, accumulate, accumulate ? out[o] : 0.0f);
            }
        }
    return 0;
}

// k_conv2d_real's thread per (output pixel, group of 8 output channels).  staged != 0: the group's filters in the kernel's LDS
// layout ([(ky, kx, ci)][8], zero for a channel beyond Cout), built as the kernel builds it.
extern "C" int hostcheck_conv2d_real(const float *W, const float *bias, const float *x, float *out, int B, int Cin, int H, int Wd, int Cout,
                                     int KH, int KW, int stride, int pad, int accumulate, int staged) {
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (Wd + 2 * pad - KW) / stride + 1, taps = Cin * KH * KW;
    if (OH <= 0 || OW <= 0) return -1;
    std::vector<float> wsm((size_t)taps * 8);
    for (int c0 = 0; c0 < Cout; c0 += 8) {
        for (int k = 0; k < taps * 8; ++k) {
            const int o = k >> 3, u = k & 7, ci = o % Cin, kk = o / Cin;
            wsm[k] = c0 + u < Cout ? W[((size_t)(c0 + u) * Cin + ci) * KH * KW + kk] : 0.0f;
        }
        for (int b = 0; b < B; ++b)
            for (int oy = 0; oy < OH; ++oy)
                for (int ox = 0; ox < OW; ++ox) {
                    const float *sb = x + (size_t)b * Cin * H * Wd;
                    float acc[8];
                    real_conv2d_chains<8>(acc,
                        [&](int ci, int iy, int ix) { return sb[((size_t)ci * H + iy) * Wd + ix]; },
                        [&](int u, int ci, int ky, int kx) {
                            if (staged) return wsm[((size_t)(ky * KW + kx) * Cin + ci) * 8 + u];
                            return c0 + u < Cout ? W[(((size_t)(c0 + u) * Cin + ci) * KH + ky) * KW + kx] : 0.0f;
                        }, Cin, H, Wd, KH, KW, stride, pad, oy, ox);
                    for (int u = 0; u < 8 && c0 + u < Cout; ++u) {
                        const size_t o = (((size_t)b * Cout + c0 + u) * OH + oy) * OW + ox;
                        out[o] = real_finish(acc[u], bias != nullptr, bias ? bias[c0 + u] : 0.0f, accumulate, accumulate ? out[o] : 0.0f);
                    }
                }
    }
    return 0;
}

// k_input_real's thread per element, T steps.  s [T, B, N]; decay_vec / scale_vec nullable [N] (the per-neuron rows); xrec [T, B, N].
extern "C" void hostcheck_input_real(const float *s, float *x, int T, int B, int N, float decay, float scale, int additive,
                                     const float *decay_vec, const float *scale_vec, float *xrec) {
    snn_lif_params p = {};
    p.traces = 1; p.trace_decay = decay; p.trace_scale = scale; p.traces_additive = additive;
    snn_pervec pv = {};
    pv.v[SNN_PV_TRACE_DECAY] = decay_vec;
    pv.v[SNN_PV_TRACE_SCALE] = scale_vec;
    for (int t = 0; t < T; ++t)
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < N; ++j) {
                const size_t k = (size_t)b * N + j;
                const node_row r = row_of<true>(p, 0.f, pv, j);
                x[k] = real_trace_next(x[k], s[(size_t)t * B * N + k], r.trace_decay, r.trace_scale, additive);
                xrec[(size_t)t * B * N + k] = x[k];
            }
}
