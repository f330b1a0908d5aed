// Host-side check of bindsnet_amd/csrc/snn_convnd.hpp: the __host__ __device__ bodies of the Conv1d / Conv3d propagation chain
// and of the PostPre element sums are run HERE on the CPU (compiled by hipcc like the kernels, no device code is executed), one
// output or weight element at a time, exactly as k_prop_convnd's and k_convnd_postpre's threads call them.  Test infrastructure
// only (tests/test_conv_nd_host.py); not part of libsnnhip.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_convnd.hpp"

// out [B, Cout, OD, OH, OW] = chain + bias (bias nullable), s [B, Cin, D, H, Wd] 0/1 bytes, W [Cout, Cin, KD, KH, KW]
extern "C" int hostcheck_convnd_prop(const float *W, const float *bias, const uint8_t *s, int B, int Cin, int D, int H, int Wd, int Cout,
                                     int KD, int KH, int KW, int stride, int pad, float *out) {
    const snn::ConvNdGeom g = snn::convnd_geom(Cin, D, H, Wd, Cout, KD, KH, KW, stride, pad);
    const int OH = g.OH, OW = g.OW;
    const long n_src = (long)Cin * D * H * Wd, P = (long)g.OD * OH * OW, taps = (long)Cin * KD * KH * KW;
    for (int b = 0; b < B; ++b) {
        std::vector<uint32_t> bits((n_src + 31) / 32);
        for (long k = 0; k < (long)bits.size(); ++k) bits[k] = snn::convnd_pack_word(s + b * n_src, g, k, n_src);
        for (int co = 0; co < Cout; ++co)
            for (long p = 0; p < P; ++p) {
                const int ow = (int)(p % OW), oh = (int)((p / OW) % OH), od = (int)(p / ((long)OW * OH));
                const float *wf = W + co * taps;
                const float acc = snn::convnd_chain(g, od, oh, ow, [&](long k) { return bits[k]; }, [&](int i) { return wf[i]; });
                out[((long)b * Cout + co) * P + p] = bias ? acc + bias[co] : acc;
            }
    }
    return 0;
}

// per-sample element sums: pre / post [B, Cout, J]; tab [L, J]; s_src / x_src [B, n_src]; s_tgt / x_tgt [B, Cout, L]
extern "C" int hostcheck_convnd_pp(const int *tab, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                                   int Cout, int L, int J, int n_src, float *pre, float *post) {
    const int nw = (L + 31) / 32;
    for (int b = 0; b < B; ++b)
        for (int co = 0; co < Cout; ++co) {
            std::vector<uint32_t> mk(nw);
            for (int k = 0; k < nw; ++k) mk[k] = snn::convnd_pack_row_word(s_tgt + ((long)b * Cout + co) * L, L, k);
            for (int j = 0; j < J; ++j) {
                const long id = ((long)b * Cout + co) * J + j;
                pre[id] = snn::convnd_pp_pre(tab, L, J, j, x_tgt + ((long)b * Cout + co) * L,
                                             [&](int i) { return (float)s_src[(long)b * n_src + i]; });
                post[id] = snn::convnd_pp_post(tab, L, J, j, [&](int k) { return mk[k]; },
                                               [&](int i) { return x_src[(long)b * n_src + i]; });
            }
        }
    return 0;
}
