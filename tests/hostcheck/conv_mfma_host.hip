// The bodies of bindsnet_amd/csrc/snn_conv_mfma.hpp on the CPU with k_conv_mfma's schedule (block of 64 pixels, group of 16 NT channels,
// slab of 64 padded terms); the MFMA is the fmaf chain it is documented to be.  For tests/test_conv_mfma_hostcheck.py; not in libsnnhip.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_conv_mfma.hpp"

using namespace snn;
namespace cm = snn::conv_mfma;

// counters: blocks x groups through {chain, scalar body}.  Valid arguments only; 0, or -3 for a tap offset outside its staged band
extern "C" int hostcheck_conv_mfma(const float *W, const float *bias, const uint8_t *s, float *out, int B, int Cin, int H, int Wd, int Cout,
                                   int KH, int KW, int stride, int pad, int accumulate, int NT, int *counters) {
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (Wd + 2 * pad - KW) / stride + 1;
    const WideGeom g = {Cin, H, Wd, KH, KW, stride, pad, OH, OW, Cout};
    const int nps = OH * OW, ps = wide_pixel_stride(Cin), CPB = cm::padded_channels(Cin) / 16, RS = cm::slab_stride(NT), G = 16 * NT;
    const int nslab = (KH * KW * CPB + 3) / 4;
    const long npix = (long)B * nps;
    const size_t img = (size_t)Cin * H * Wd, slot_bytes = (size_t)cm::band_bytes(g);
    std::vector<WideQuad> bands((size_t)cm::block_samples(nps, B) * slot_bytes / 16 + 1);
    std::vector<float> slab((size_t)cm::slab_floats(NT)), acc((size_t)cm::kBlockPix * G);
    uint8_t *bb = (uint8_t *)bands.data();
    for (long p0 = 0; p0 < npix; p0 += cm::kBlockPix) {
        const long plast = p0 + cm::kBlockPix - 1 < npix - 1 ? p0 + cm::kBlockPix - 1 : npix - 1;
        const int bfirst = (int)(p0 / nps), nsm = (int)(plast / nps) - bfirst + 1;
        dense_auto::census cen = {0, 0};
        for (int sm = 0; sm < nsm; ++sm)
            cm::stage_band((uint32_t *)(bb + sm * slot_bytes), s + (size_t)(bfirst + sm) * img, g, cm::band_of(p0, npix, bfirst + sm, g), 0, 1, cen);
        for (int c0 = 0; c0 < Cout; c0 += G) {
            counters[cen.above1 ? 1 : 0] += 1;
            for (float &a : acc) a = 0.f;
            for (int sl = 0; sl < nslab && !cen.above1; ++sl) {
                for (int e = 0; e < cm::kSlabRows * G; ++e) {
                    const cm::SlabSlot at = cm::slab_slot(e);
                    slab[(size_t)at.row * RS + at.col] = cm::slab_weight(W, g, (long long)sl * cm::kSlabRows + at.row, c0 + at.col);
                }
                for (long p = p0; p <= plast; ++p) {
                    const int b = (int)(p / nps), pin = (int)(p - (long)b * nps), oy = pin / OW, ox = pin - oy * OW;
                    const cm::Band band = cm::band_of(p0, npix, b, g);
                    for (int j = 0; j < 4; ++j) {
                        const int rd = sl * 4 + j, kk = rd / CPB, cb = rd - kk * CPB;
                        const int off = kk < KH * KW ? cm::tap_offset(g, band, oy, ox, kk / KW, kk % KW) : -1;
                        if (off >= 0 && (size_t)off + ps > (size_t)band.rows * Wd * ps) return -3;
                        const WideQuad q = off >= 0 ? *(const WideQuad *)(bb + (b - bfirst) * slot_bytes + off + cb * 16) : WideQuad{{0u, 0u, 0u, 0u}};
                        for (int u = 0; u < 4; ++u)
                            for (int kq = 0; kq < 4; ++kq)
                                for (float *a = &acc[(size_t)(p - p0) * G], *w = &slab[(size_t)(j * 16 + 4 * u + kq) * RS], *e = a + G; a < e; ++a, ++w)
                                    *a = __builtin_fmaf(cm::spike_of(q, u, kq), *w, *a);
                    }
                }
            }
            for (long p = p0; p <= plast; ++p) {
                const int b = (int)(p / nps), pin = (int)(p - (long)b * nps), oy = pin / OW, ox = pin - oy * OW;
                for (int c = 0; c < G && c0 + c < Cout; ++c) {
                    float a = acc[(size_t)(p - p0) * G + c];
                    if (cen.above1) a = cm::scalar_output(bb + (b - bfirst) * slot_bytes, cm::band_of(p0, npix, b, g), g, oy, ox, W, c0 + c);
                    const size_t o = ((size_t)b * Cout + c0 + c) * nps + pin;
                    out[o] = wide_emit(a, bias, c0 + c, accumulate ? out[o] : 0.0f, accumulate);
                }
            }
        }
    }
    return 0;
}
