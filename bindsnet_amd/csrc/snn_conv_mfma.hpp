// snn_conv_mfma.hpp -- the order-carrying bodies of snn_prop_conv2d_mfma_f32 (csrc/snn_conv_mfma.hip): Conv2dConnection.compute over
// spike bytes as an implicit GEMM on v_mfma_f32_16x16x4_f32.  M = the output pixels of the flattened [B, OH, OW], N = Cout, K = the
// ordered taps; A[m][q] is a spike byte (or 0), B[q][co] = W[co][ci][ky][kx].
//
// Stated order (include/snnhip.h, snn_prop_conv2d_f32): every output is ONE sequential f32 sum over q = (ky * KW + kx) * Cin + ci, an
// out-of-image tap skipped, a zero byte adding nothing, every other adding f32(byte) * w with a rounded multiply and a rounded add;
// the bias last.  gfx950's f32-input MFMA is a k-ordered fmaf chain (csrc/snn_mfma.hip), so ONE accumulator per 16x16 output tile,
// carried from the first tap to the last, walks that order.  Why the bits agree:
//   * a byte of 1: fma(1, w, acc) is round(acc + w), the rounded add of the exact product w (snn_dense_auto.hpp, chain_fma);
//   * a byte of 0, a tap outside the image (the lane feeds 0 without reading) and a PADDED term: the walk pads every tap's channels to
//     a multiple of 16, so that a round of four MFMAs is 16 channels of one tap; a padded term has spike 0 AND weight 0.  All of these
//     add fma(0, w, acc) = acc + (+-0).  A chain that started at +0 is never -0 (x + y is -0 only if both are -0, and round-to-nearest
//     gives +0 for x + (-x)), so adding +-0 leaves every bit of acc -- for finite w.  A non-finite weight under a silent tap gives
//     0 * inf = NaN here, where the stated order skips it;
//   * a byte above 1: fma rounds once, the stated order twice.  The workgroup takes the census of the bytes it staged
//     (dense_auto::census_word) and, if any is above 1, computes its outputs with scalar_output below instead.
// The sum is cut into consecutive slabs of kSlabRows padded terms (a sequential sum cut into consecutive pieces is the same sum); the
// accumulators stay in registers across the cuts.
//
// LDS of a workgroup (4 waves: 4 consecutive tiles of 16 output pixels x NT tiles of 16 output channels per wave, the waves sharing
// the channel group):
//   * two weight slabs [kSlabRows][slab_stride(NT)] floats, row = padded term, column = channel of the group.  An MFMA's B operand is
//     4 rows (k = lane >> 4) x 16 columns (lane & 15): banks (row * stride + column) mod 64.  stride = (NT | 1) * 16 is 16 or 48 mod 64,
//     so the 4 rows start at 4 different multiples of 16 and the 64 lanes hit 64 distinct banks.  The same holds for the transposing
//     write, whose lanes are 4 rows x 16 columns too (slab_slot);
//   * per sample the block touches, the BAND of input rows its pixels read, channels last as in snn_conv_wide.hpp (wide_stage_word,
//     wide_pixel_stride: an odd number of 16-byte units per pixel, padding bytes 0): a lane takes the 16 channels of (its pixel, this
//     tap) with one 16-byte read.
// The bodies are __host__ __device__: tests/hostcheck/conv_mfma_host.hip drives them block by block (tests/test_conv_mfma_hostcheck.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "snn_conv_wide.hpp"
#include "snn_dense_auto.hpp"

namespace snn {
namespace conv_mfma {

constexpr int kTile = 16;                        // M, N of the MFMA
constexpr int kWaves = 4;
constexpr int kBlockPix = kTile * kWaves;        // consecutive output pixels per workgroup
constexpr int kSlabRows = 64;                    // padded terms per weight slab: 4 rounds of four MFMAs
constexpr int kLdsLimit = 150 * 1024;            // the most dynamic LDS a launch asks for: gfx950 gives a workgroup 160 KiB, the kernel's
                                                 //  static LDS (the barrier's reduction words) and the runtime's share come out of the rest

__host__ __device__ __forceinline__ int padded_channels(int Cin) { return (Cin + 15) & ~15; }
__host__ __device__ __forceinline__ long long padded_terms(const WideGeom &g) { return (long long)g.KH * g.KW * padded_channels(g.Cin); }
__host__ __device__ constexpr int slab_stride(int NT) { return (NT | 1) * 16; }                   // floats per slab row
__host__ __device__ constexpr int slab_floats(int NT) { return kSlabRows * slab_stride(NT); }

// how many samples a block of kBlockPix consecutive output pixels can touch
__host__ __device__ __forceinline__ int block_samples(int npix_sample, int B) {
    const int n = (kBlockPix - 1) / npix_sample + 2;
    return n < B ? n : B;
}

// the most input rows a block reads of ONE sample: its pixels span at most floor((OW + kBlockPix - 2) / OW) + 1 output rows
__host__ __device__ __forceinline__ int band_rows_max(const WideGeom &g) {
    int span = (g.OW + kBlockPix - 2) / g.OW + 1;
    if (span > g.OH) span = g.OH;
    const long long rows = (long long)(span - 1) * g.stride + g.KH;
    return rows < g.H ? (int)rows : g.H;
}
// bytes of one sample's slot (every slot has the size of the largest band)
__host__ __device__ __forceinline__ unsigned long long band_bytes(const WideGeom &g) {
    return (unsigned long long)band_rows_max(g) * g.Wd * wide_pixel_stride(g.Cin);
}
// dynamic LDS of a launch: two slabs, then the slots (at least one 16-byte unit: a lane whose tap is outside reads nothing, but the
// region is never empty)
__host__ __device__ __forceinline__ unsigned long long lds_bytes(const WideGeom &g, int B, int NT) {
    const unsigned long long bands = (unsigned long long)block_samples(g.OH * g.OW, B) * band_bytes(g);
    return 2ull * slab_floats(NT) * sizeof(float) + (bands < 16 ? 16 : bands);
}

struct Band {
    int iy0, rows;                               // input rows iy0 .. iy0 + rows - 1 of the sample are staged
};

// the band of sample b for the block of output pixels p0 .. p0 + kBlockPix - 1 (npix = B * OH * OW)
__host__ __device__ __forceinline__ Band band_of(long p0, long npix, int b, const WideGeom &g) {
    const long nps = (long)g.OH * g.OW, s0 = (long)b * nps;
    long lo = p0 > s0 ? p0 : s0, hi = p0 + kBlockPix - 1;
    if (hi > npix - 1) hi = npix - 1;
    if (hi > s0 + nps - 1) hi = s0 + nps - 1;
    if (hi < lo) return {0, 0};
    const int oya = (int)((lo - s0) / g.OW), oyb = (int)((hi - s0) / g.OW);
    const long long a = (long long)oya * g.stride - g.pad, z = (long long)oyb * g.stride - g.pad + g.KH - 1;
    const int iy0 = a < 0 ? 0 : a > g.H ? g.H : (int)a, iy1 = z > g.H - 1 ? g.H - 1 : (int)z;
    return {iy0, iy1 >= iy0 ? iy1 - iy0 + 1 : 0};
}

// The tap map: the byte offset, inside its sample's slot, of the 16-byte units of input pixel (oy * stride - pad + ky, ox * stride -
// pad + kx), or -1 where that pixel is outside the image (the lane then feeds zeros and reads nothing).
__host__ __device__ __forceinline__ int tap_offset(const WideGeom &g, const Band &band, int oy, int ox, int ky, int kx) {
    const int iy = oy * g.stride - g.pad + ky, ix = ox * g.stride - g.pad + kx;
    if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.Wd) return -1;
    return ((iy - band.iy0) * g.Wd + ix) * wide_pixel_stride(g.Cin);
}

// Band staging: thread `tid` of `nthreads` writes its words of sample `sp`'s band ([Cin, H * Wd] bytes) into `slot` and adds them to
// its census.  Consecutive threads take consecutive pixels of one channel word, so the four byte loads of a word are coalesced.
__host__ __device__ __forceinline__ void stage_band(uint32_t *slot, const uint8_t *sp, const WideGeom &g, const Band &band, int tid,
                                                    int nthreads, dense_auto::census &c) {
    const int words = wide_pixel_stride(g.Cin) / 4, npx = band.rows * g.Wd, n = npx * words, first = band.iy0 * g.Wd;
    for (int k = tid; k < n; k += nthreads) {
        const int pix = k % npx, cw = k / npx;
        const uint32_t v = wide_stage_word(sp, g.Cin, g.H * g.Wd, first + pix, cw);
        slot[(size_t)pix * words + cw] = v;
        dense_auto::census_word(v, c);
    }
}

// The slab slot of element e of the kSlabRows x 16 NT elements a workgroup moves per slab: a wave's 64 lanes are 4 rows x 16 columns.
// Reading: 16 channels' rows of W, 4 consecutive input channels each (KH * KW floats apart; the rest of every cache line is what the
// other taps' slabs take).  Writing: 64 distinct banks (see above).
struct SlabSlot {
    int row, col;
};
__host__ __device__ __forceinline__ SlabSlot slab_slot(int e) {
    const int rest = e >> 6;
    return {(rest % (kSlabRows / 4)) * 4 + (e & 3), (rest / (kSlabRows / 4)) * 16 + ((e >> 2) & 15)};
}

// the weight at (padded term qp, output channel co): 0 for a padded channel, past the last tap and beyond Cout; W [Cout, Cin, KH * KW]
__host__ __device__ __forceinline__ float slab_weight(const float *W, const WideGeom &g, long long qp, int co) {
    const int CP = padded_channels(g.Cin), KK = g.KH * g.KW;
    const long long kk = qp / CP;
    const int ci = (int)(qp - kk * CP);
    const bool live = co < g.Cout && ci < g.Cin && kk < KK;
    const float w = W[live ? ((size_t)co * g.Cin + ci) * KK + (size_t)kk : 0];      // (always a valid address: no branch around the load)
    return live ? w : 0.0f;
}

// byte 4 u + kq of the 16 channels in `q`, as the A operand of the round's MFMA u (the spikes() of snn_mfma.hip)
__host__ __device__ __forceinline__ float spike_of(const WideQuad &q, int u, int kq) { return (float)((q.w[u] >> (8 * kq)) & 0xFFu); }

// The scalar body: output (pixel (oy, ox), channel co) in the stated order from the staged band -- one rounded multiply and one
// rounded add per non-zero byte (-ffp-contract=off), zero bytes and out-of-image taps skipped.  Slow and exact for any byte.
__host__ __device__ __forceinline__ float scalar_output(const uint8_t *slot, const Band &band, const WideGeom &g, int oy, int ox,
                                                        const float *W, int co) {
    const int KK = g.KH * g.KW;
    const float *Wc = W + (size_t)co * g.Cin * KK;
    float acc = 0.0f;
    for (int ky = 0; ky < g.KH; ++ky)
        for (int kx = 0; kx < g.KW; ++kx) {
            const int off = tap_offset(g, band, oy, ox, ky, kx);
            if (off < 0) continue;
            for (int ci = 0; ci < g.Cin; ++ci) {
                const uint8_t sv = slot[off + ci];
                if (!sv) continue;
                const float t = (float)sv * Wc[(size_t)ci * KK + ky * g.KW + kx];
                acc = acc + t;
            }
        }
    return acc;
}

}  // namespace conv_mfma
}  // namespace snn
