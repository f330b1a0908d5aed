// snn_conv_wide.hip -- Conv2dConnection.compute for the shapes k_conv2d (snn_ops.hip) does not take: more than 16 input channels, or a
// filter bank beyond 64 KiB.  The order, the LDS layouts and the event-driven skips are described in snn_conv_wide.hpp, whose bodies
// this kernel calls; snn_prop_conv2d_f32 (snn_ops.hip) routes here.
//
// grid (blocks of 256 consecutive output pixels of the flattened [B, OH, OW], chunks of 8 output channels), 256 threads: thread <->
// output pixel.  A workgroup stages the images of the samples its pixels belong to once (channels last), then per chunk walks the
// ordered taps slab by slab: stage the slab's weights for its 8 channels, accumulate, next slab.  More chunks than gridDim.y can
// hold are looped over.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_conv_wide.hpp"

using namespace snn;

template <bool STAGED>
__global__ __launch_bounds__(kWideThreads) void k_conv_wide(const float *__restrict__ W, const float *__restrict__ bias,
                                                            const uint8_t *__restrict__ s, float *__restrict__ out, int B, WideGeom g,
                                                            int accumulate, int nstage) {
    extern __shared__ __align__(16) unsigned char wide_lds[];
    float *wslab = (float *)wide_lds;                                               // [kWideSlabTaps][kWideCC]
    uint8_t *simg = wide_lds + sizeof(float) * kWideSlabTaps * kWideCC;             // [nstage][H * Wd][ps], STAGED only
    const int tid = threadIdx.x;
    const int taps = g.Cin * g.KH * g.KW, hw = g.H * g.Wd, npix_s = g.OH * g.OW, ps = wide_pixel_stride(g.Cin);
    const size_t img = (size_t)g.Cin * hw;
    const long npix = (long)B * npix_s, p0 = (long)blockIdx.x * kWideThreads, p = p0 + tid;
    const int bfirst = (int)(p0 / npix_s);
    if (STAGED) {
        const int nst = min(nstage, B - bfirst), words = ps / 4, n = nst * words * hw;
        for (int k = tid; k < n; k += kWideThreads) {                               // consecutive threads: consecutive pixels of one channel word
            const int pix = k % hw, r = k / hw, cw = r % words, sm = r / words;
            ((uint32_t *)simg)[((size_t)sm * hw + pix) * words + cw] = wide_stage_word(s + (size_t)(bfirst + sm) * img, g.Cin, hw, pix, cw);
        }
    }
    const bool valid = p < npix;
    const long pc = valid ? p : npix - 1;
    const int ox = (int)(pc % g.OW), oy = (int)((pc / g.OW) % g.OH), b = (int)(pc / npix_s);
    const uint8_t *sp = STAGED ? simg + (size_t)(b - bfirst) * hw * ps : s + (size_t)b * img;
    const int nchunk = (g.Cout + kWideCC - 1) / kWideCC;
    for (int chunk = blockIdx.y; chunk < nchunk; chunk += gridDim.y) {
        const int c0 = chunk * kWideCC;
        float acc[kWideCC];
#pragma unroll
        for (int u = 0; u < kWideCC; ++u) acc[u] = 0.f;
        for (int q0 = 0; q0 < taps; q0 += kWideSlabTaps) {
            const int q1 = min(q0 + kWideSlabTaps, taps);
            __syncthreads();                                                        // the previous slab has been read (first pass: the images are staged)
            for (int e = tid; e < (q1 - q0) * kWideCC; e += kWideThreads) wslab[e] = wide_slab_weight(W, g, c0, q0, e);
            __syncthreads();
            wide_accumulate<STAGED>(acc, sp, valid, oy, ox, g, wslab, q0, q1);
        }
        if (valid) {
#pragma unroll
            for (int u = 0; u < kWideCC; ++u)
                if (c0 + u < g.Cout) {
                    const size_t o = (((size_t)b * g.Cout + c0 + u) * g.OH + oy) * g.OW + ox;
                    out[o] = wide_emit(acc[u], bias, c0 + u, accumulate ? out[o] : 0.0f, accumulate);
                }
        }
    }
}

// Called by snn_prop_conv2d_f32 with checked arguments (all positive, OH and OW from the geometry).
int snn_conv_wide_launch(const float *W, const float *bias, const uint8_t *s, float *out, int B, int Cin, int H, int Wd, int Cout,
                         int KH, int KW, int stride, int pad, int OH, int OW, int accumulate, hipStream_t stream) {
    // index widths: the ordered tap index, the image offset of a sample and the output pixel of a sample are ints, the pixel blocks gridDim.x
    if ((long long)Cin * KH * KW > SNN_CONV2D_MAX_TAPS || (long long)Cin * H * Wd > SNN_CONV2D_MAX_IMAGE ||
        (long long)OH * OW > SNN_CONV2D_MAX_IMAGE)
        return SNN_ERR_UNSUPPORTED;
    const long long blocks = ((long long)B * OH * OW + kWideThreads - 1) / kWideThreads;
    if (blocks > 0x7fffffffll) return SNN_ERR_UNSUPPORTED;
    WideGeom g = {Cin, H, Wd, KH, KW, stride, pad, OH, OW, Cout};
    const int nchunk = (Cout + kWideCC - 1) / kWideCC;
    const dim3 grid((unsigned)blocks, (unsigned)(nchunk < 65535 ? nchunk : 65535));
    const size_t slab = sizeof(float) * kWideSlabTaps * kWideCC;
    const int nstage = wide_block_samples(OH * OW, B);
    const unsigned long long stage = (unsigned long long)nstage * H * Wd * wide_pixel_stride(Cin);
    if (stage <= (unsigned long long)kWideStageBytes)
        hipLaunchKernelGGL(k_conv_wide<true>, grid, dim3(kWideThreads), slab + (size_t)stage, stream, W, bias, s, out, B, g, accumulate, nstage);
    else
        hipLaunchKernelGGL(k_conv_wide<false>, grid, dim3(kWideThreads), slab, stream, W, bias, s, out, B, g, accumulate, 0);
    return snn_check_launch();
}
