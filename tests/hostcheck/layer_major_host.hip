// The bodies of bindsnet_amd/csrc/snn_run_conv_sif.hpp on the CPU: k_run_conv_sif's time loop as its per-step scalar restatement (band
// staging word by word, conv_mfma::scalar_output in the stated tap order, neuron_step) with the kernel's split -- sample, block of 64
// output pixels, group of 16 channels -- and k_sif_scan's body.  For tests/test_layer_major_hostcheck.py; not in libsnnhip.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_run_conv_sif.hpp"

using namespace snn;
namespace cm = snn::conv_mfma;
namespace rcs = snn::run_conv;

static snn_lif_params params(float thresh, float refrac, float dt, int has_lbound, float lbound, int traces, float trace_decay, float trace_scale) {
    snn_lif_params p = {};
    p.thresh = thresh, p.refrac = refrac, p.dt = dt, p.has_lbound = has_lbound, p.lbound = lbound;
    p.traces = traces, p.trace_decay = trace_decay, p.trace_scale = trace_scale, p.traces_additive = 0;
    return p;
}

// 0, or -3 for a band word or a tap outside its slot
extern "C" int hostcheck_run_conv_sif(const float *W, const float *bias, const uint8_t *s0, const uint8_t *s_train, uint8_t *out_train, float *v,
                                      float *refrac, float *summed, float *x, uint8_t *s, int T, int B, int Cin, int H, int Wd, int Cout, int KH,
                                      int KW, int stride, int pad, float thresh, float refrac_p, float dt, int has_lbound, float lbound, int traces,
                                      float trace_decay, float trace_scale) {
    const snn_lif_params p = params(thresh, refrac_p, dt, has_lbound, lbound, traces, trace_decay, trace_scale);
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (Wd + 2 * pad - KW) / stride + 1, nps = OH * OW;
    const WideGeom g = {Cin, H, Wd, KH, KW, stride, pad, OH, OW, Cout};
    const size_t img = (size_t)Cin * H * Wd, slot_bytes = (size_t)(rcs::bands_bytes(g) / 2);
    std::vector<uint32_t> slot(slot_bytes / 4 + 4);
    for (int b = 0; b < B; ++b)
        for (int p0 = 0; p0 < nps; p0 += cm::kBlockPix) {
            const cm::Band band = rcs::block_band(p0, g);
            const int nwords = rcs::band_words(g, band);
            if ((size_t)nwords * 4 > slot_bytes) return -3;
            for (int t = 0; t < T; ++t) {
                const uint8_t *sp = (t == 0 ? s0 : s_train + (size_t)(t - 1) * B * img) + (size_t)b * img;
                for (int k = 0; k < nwords; ++k) {
                    const int at = rcs::band_word_slot(g, band, k);
                    if (at < 0 || at >= nwords) return -3;
                    slot[at] = rcs::band_word(sp, g, band, k);
                }
                for (int pp = p0; pp < p0 + cm::kBlockPix && pp < nps; ++pp)
                    for (int co = 0; co < Cout; ++co) {
                        const size_t n = ((size_t)b * Cout + co) * nps + pp;
                        const float acc = cm::scalar_output((const uint8_t *)slot.data(), band, g, pp / OW, pp % OW, W, co);
                        float unused = 0.f;
                        s[n] = out_train[(size_t)t * B * Cout * nps + n] =
                            rcs::neuron_step(acc, bias, co, v[n], refrac[n], summed != nullptr, summed ? summed[n] : unused, x ? x[n] : unused, p);
                    }
            }
        }
    return 0;
}

extern "C" int hostcheck_sif_scan(float *v, float *refrac, uint8_t *s, float *x, float *summed, const float *I, uint8_t *train, int Tc, int B, int N,
                                  float thresh, float refrac_p, float dt, int has_lbound, float lbound, int traces, float trace_decay,
                                  float trace_scale) {
    const snn_lif_params p = params(thresh, refrac_p, dt, has_lbound, lbound, traces, trace_decay, trace_scale);
    const long n = (long)B * N;
    for (long k = 0; k < n; ++k) {
        float unused = 0.f;
        s[k] = rcs::scan_neuron(v[k], refrac[k], summed != nullptr, summed ? summed[k] : unused, x ? x[k] : unused, I + k, train + k, Tc, n, p);
    }
    return 0;
}
