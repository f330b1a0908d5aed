// snn_conv_wide.hpp -- the order-carrying bodies of Conv2dConnection.compute for the shapes k_conv2d (snn_ops.hip) does not take:
// more than 16 input channels, or a filter bank beyond 64 KiB.
//
// Stated order (include/snnhip.h, snn_prop_conv2d_f32; oracle/snn_oracle.c, orc_prop_conv2d): every output element is ONE
// sequential f32 sum over the ordered taps q = (ky * KW + kx) * Cin + ci -- taps row-major, input channels innermost --, a tap
// outside the image is skipped, a tap whose spike byte is 0 adds nothing, every other adds f32(byte) * w with one rounded multiply
// and one rounded add (no FMA: -ffp-contract=off); the bias is added last.
//
// The kernel (snn_conv_wide.hip) gives a thread one output pixel and kWideCC consecutive output channels, and walks the ordered taps
// in consecutive slabs of kWideSlabTaps: a sequential sum cut into consecutive pieces is the same sum.  Per slab the workgroup holds
//   * the weights in LDS as wslab[(q - q0) * kWideCC + u]: all lanes of a wave walk the taps together, so the kWideCC floats of a
//     tap are one address for the whole wave -- two 16-byte broadcast reads, free of bank conflicts whatever the lanes' pixels are;
//   * the images of the block's samples in LDS, channels last: the byte of (ci, iy, ix) at (iy * Wd + ix) * ps + ci with
//     ps = wide_pixel_stride(Cin) bytes, an ODD number of 16-byte units (padding bytes 0).  A lane reads 16 channels of its pixel with
//     one 16-byte read; neighbouring lanes are neighbouring pixels, an odd number of units apart, so 16 lanes cover all 64 banks.
//     A sample's image that does not fit is read from global memory byte by byte (STAGED = false).
// Event-driven: a tap position outside the image for every lane of the wave, a group of 16 channels silent for every lane and a tap
// silent for every lane are skipped without touching the weights (wide_any); a lane adds only where its own byte is set.
//
// The bodies are __host__ __device__: tests/hostcheck/conv_wide_host.hip drives them on the CPU block by block and slab by slab as the
// kernel does (tests/test_conv_wide_hostcheck.py); there wide_any is the lane's own predicate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snn {

constexpr int kWideThreads = 256;                // output pixels per workgroup
constexpr int kWideCC = 8;                       // output channels per workgroup
constexpr int kWideSlabTaps = 512;               // ordered taps per weight slab: 512 * 8 * 4 = 16 KiB of LDS
constexpr int kWideStageBytes = 48 * 1024;       // LDS for the staged images; with the slab 64 KiB, the default limit of a launch

struct WideGeom {
    int Cin, H, Wd, KH, KW, stride, pad, OH, OW, Cout;
};

struct alignas(16) WideQuad {                    // 16 channels of one pixel
    uint32_t w[4];
};

// bytes between two pixels of a staged image: ceil(Cin / 16) 16-byte units, made odd
__host__ __device__ __forceinline__ int wide_pixel_stride(int Cin) { return (((Cin + 15) / 16) | 1) * 16; }

// how many samples a block of kWideThreads consecutive output pixels can touch
__host__ __device__ __forceinline__ int wide_block_samples(int npix_sample, int B) {
    const int n = (kWideThreads - 1) / npix_sample + 2;
    return n < B ? n : B;
}

// true where the predicate holds for any lane of the wave (all lanes of a workgroup reach every call: none leaves the tap walk)
__host__ __device__ __forceinline__ bool wide_any(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __any((int)p) != 0;
#else
    return p;
#endif
}

// word `cw` (channels 4 cw .. 4 cw + 3, low byte first, 0 beyond Cin) of pixel `pix` of a staged image; s: the sample, [Cin, H * Wd]
__host__ __device__ __forceinline__ uint32_t wide_stage_word(const uint8_t *s, int Cin, int hw, int pix, int cw) {
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = 4 * cw + j;
        if (ci < Cin) v |= (uint32_t)s[(size_t)ci * hw + pix] << (8 * j);
    }
    return v;
}

// element e of the slab of ordered taps [q0, q1) for output channels c0 .. c0 + kWideCC - 1 (0 beyond Cout); W [Cout, Cin, KH * KW]
__host__ __device__ __forceinline__ float wide_slab_weight(const float *W, const WideGeom &g, int c0, int q0, int e) {
    const int u = e % kWideCC, q = q0 + e / kWideCC, co = c0 + u;
    if (co >= g.Cout) return 0.0f;
    const int kk = q / g.Cin, ci = q - kk * g.Cin;
    return W[((size_t)co * g.Cin + ci) * ((size_t)g.KH * g.KW) + kk];
}

__host__ __device__ __forceinline__ void wide_add(float (&acc)[kWideCC], uint32_t sv, const float *w) {
    const float fs = (float)sv;
#pragma unroll
    for (int u = 0; u < kWideCC; ++u) acc[u] += fs * w[u];
}

// The ordered taps [q0, q1) of output pixel (oy, ox) into acc.  sp: the pixel's sample -- STAGED: its channels-last image, else its
// [Cin, H, Wd] bytes in global memory.  valid: false for the lanes behind the last pixel, which walk along and add nothing.
template <bool STAGED>
__host__ __device__ __forceinline__ void wide_accumulate(float (&acc)[kWideCC], const uint8_t *sp, bool valid, int oy, int ox,
                                                         const WideGeom &g, const float *wslab, int q0, int q1) {
    const int ps = wide_pixel_stride(g.Cin);
    for (int kk = q0 / g.Cin; kk < g.KH * g.KW && kk * g.Cin < q1; ++kk) {
        const int ky = kk / g.KW, kx = kk - ky * g.KW;
        const int iy = oy * g.stride - g.pad + ky, ix = ox * g.stride - g.pad + kx;
        const bool in = valid && iy >= 0 && iy < g.H && ix >= 0 && ix < g.Wd;
        if (!wide_any(in)) continue;
        const int base = kk * g.Cin - q0;                                  // slab position of channel 0 of this tap (may be negative)
        const int c_lo = base < 0 ? -base : 0, c_hi = q1 - kk * g.Cin < g.Cin ? q1 - kk * g.Cin : g.Cin;
        if (STAGED) {
            const uint8_t *px = sp + (in ? (size_t)(iy * g.Wd + ix) * ps : 0);
            for (int c16 = c_lo & ~15; c16 < c_hi; c16 += 16) {
                WideQuad v = {{0u, 0u, 0u, 0u}};
                if (in) v = *(const WideQuad *)(px + c16);
                if (!wide_any((v.w[0] | v.w[1] | v.w[2] | v.w[3]) != 0u)) continue;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int ci = c16 + j;
                    const uint32_t sv = (ci >= c_lo && ci < c_hi) ? (v.w[j >> 2] >> (8 * (j & 3))) & 255u : 0u;
                    if (!wide_any(sv != 0u)) continue;
                    if (sv) wide_add(acc, sv, wslab + (size_t)(base + ci) * kWideCC);
                }
            }
        } else {
            for (int ci = c_lo; ci < c_hi; ++ci) {
                const uint32_t sv = in ? sp[((size_t)ci * g.H + iy) * g.Wd + ix] : 0u;
                if (!wide_any(sv != 0u)) continue;
                if (sv) wide_add(acc, sv, wslab + (size_t)(base + ci) * kWideCC);
            }
        }
    }
}

// out (+)= sum + bias, as k_conv2d writes it
__host__ __device__ __forceinline__ float wide_emit(float acc, const float *bias, int co, float prev, int accumulate) {
    float r = acc;
    if (bias) r = r + bias[co];
    return (accumulate ? prev : 0.0f) + r;
}

}  // namespace snn
