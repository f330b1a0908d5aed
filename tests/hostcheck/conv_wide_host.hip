// Host-side check of bindsnet_amd/csrc/snn_conv_wide.hpp: the __host__ __device__ bodies of the wide Conv2dConnection.compute kernel --
// image staging (channels last), slab staging, the ordered accumulation, the emit -- are run HERE on the CPU (compiled by hipcc like the
// kernel, no device code is executed), with k_conv_wide's own schedule: block of 256 output pixels by block, chunk of 8 output
// channels by chunk, slab of 512 ordered taps by slab, "thread" by thread.  force_global != 0 takes the unstaged path whatever the
// image size.  Test infrastructure only (tests/test_conv_wide_hostcheck.py); not part of libsnnhip.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_conv_wide.hpp"

using namespace snn;

// returns 1 if the images were staged, 0 if read from `s` directly, -1 on bad arguments
extern "C" int hostcheck_conv_wide(const float *W, const float *bias, const uint8_t *s, float *out, int B, int Cin, int H, int Wd, int Cout,
                                   int KH, int KW, int stride, int pad, int accumulate, int force_global) {
    if (B <= 0 || Cin <= 0 || H <= 0 || Wd <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0) return -1;
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (Wd + 2 * pad - KW) / stride + 1;
    if (OH <= 0 || OW <= 0) return -1;
    const WideGeom g = {Cin, H, Wd, KH, KW, stride, pad, OH, OW, Cout};
    const int taps = Cin * KH * KW, hw = H * Wd, npix_s = OH * OW, ps = wide_pixel_stride(Cin), words = ps / 4;
    const size_t img = (size_t)Cin * hw;
    const long npix = (long)B * npix_s;
    const int nstage = wide_block_samples(npix_s, B);
    const bool staged = !force_global && (unsigned long long)nstage * hw * ps <= (unsigned long long)kWideStageBytes;
    std::vector<float> wslab((size_t)kWideSlabTaps * kWideCC);
    std::vector<WideQuad> simg(staged ? (size_t)nstage * hw * ps / 16 : 1);
    std::vector<float> acc((size_t)kWideThreads * kWideCC);
    const int nchunk = (Cout + kWideCC - 1) / kWideCC;
    for (long p0 = 0; p0 < npix; p0 += kWideThreads) {
        const int bfirst = (int)(p0 / npix_s);
        if (staged) {
            const int nst = nstage < B - bfirst ? nstage : B - bfirst;
            for (int k = 0; k < nst * words * hw; ++k) {
                const int pix = k % hw, r = k / hw, cw = r % words, sm = r / words;
                ((uint32_t *)simg.data())[((size_t)sm * hw + pix) * words + cw] = wide_stage_word(s + (size_t)(bfirst + sm) * img, Cin, hw, pix, cw);
            }
        }
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            const int c0 = chunk * kWideCC;
            for (float &a : acc) a = 0.f;
            for (int q0 = 0; q0 < taps; q0 += kWideSlabTaps) {
                const int q1 = q0 + kWideSlabTaps < taps ? q0 + kWideSlabTaps : taps;
                for (int e = 0; e < (q1 - q0) * kWideCC; ++e) wslab[e] = wide_slab_weight(W, g, c0, q0, e);
                for (int tid = 0; tid < kWideThreads; ++tid) {
                    const long p = p0 + tid;
                    const bool valid = p < npix;
                    const long pc = valid ? p : npix - 1;
                    const int ox = (int)(pc % OW), oy = (int)((pc / OW) % OH), b = (int)(pc / npix_s);
                    float (&a)[kWideCC] = *(float (*)[kWideCC])(acc.data() + (size_t)tid * kWideCC);
                    if (staged) wide_accumulate<true>(a, (const uint8_t *)simg.data() + (size_t)(b - bfirst) * hw * ps, valid, oy, ox, g, wslab.data(), q0, q1);
                    else wide_accumulate<false>(a, s + (size_t)b * img, valid, oy, ox, g, wslab.data(), q0, q1);
                }
            }
            for (int tid = 0; tid < kWideThreads && p0 + tid < npix; ++tid) {
                const long p = p0 + tid;
                const int ox = (int)(p % OW), oy = (int)((p / OW) % OH), b = (int)(p / npix_s);
                for (int u = 0; u < kWideCC && c0 + u < Cout; ++u) {
                    const size_t o = (((size_t)b * Cout + c0 + u) * OH + oy) * OW + ox;
                    out[o] = wide_emit(acc[(size_t)tid * kWideCC + u], bias, c0 + u, accumulate ? out[o] : 0.0f, accumulate);
                }
            }
        }
    }
    return staged ? 1 : 0;
}
