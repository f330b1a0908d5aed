// snn_run_conv_sif.hpp -- the order-carrying bodies of snn_run_conv2d_sif_f32 (csrc/snn_run_conv_sif.hip): a Conv2dConnection over spike
// bytes and the SubtractiveResetIFNodes layer it feeds, over ALL T steps of a run in one launch (the layer-major plan of Network.run).
//
// Semantics, for t = 0 .. T-1, exactly the generic plan's (snn_run.hip, run_generic): the current of step t is
// snn_prop_conv2d_f32 of the source's frame of step t-1 (the start frame for t = 0) -- one sequential f32 sum over (ky, kx, ci), the
// bias last, stored as 0 + sum (wide_emit, a lone feeder) --, then snn::sif_update and snn::sif_summed (snn_conversion.hpp), then the
// trace step of k_sif.  neuron_step below is that epilogue for one neuron; the sum is conv_mfma's: the MFMA chain where the staged
// frame is all 0/1, conv_mfma::scalar_output where it is not -- the argument for bit equality at the top of snn_conv_mfma.hpp carries
// over unchanged, because the accumulator restarts at +0 every step and the current reaches `v` through sif_update only, never
// through the MFMA's C operand.
//
// A workgroup owns kBlockPix consecutive output pixels of ONE sample and 16 output channels, for all T: band_of() is asked with the
// sample as the whole batch (npix = OH * OW, b = 0), so its band is the same rows in every frame.  LDS of a workgroup:
//   * the group's weights, [padded term][16] floats (conv_mfma's slab layout at NT = 1: stride 16, the four k rows of an MFMA's B
//     operand start 16 banks apart).  RESIDENT: every slab, transposed once; else two slabs that stream every step;
//   * two band buffers: frame t feeds the chains out of one while frame t + 1 is written to the other.
// The bodies are __host__ __device__: tests/hostcheck/layer_major_host.hip drives them (tests/test_layer_major_hostcheck.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "snn_common.hpp"
#include "snn_conv_mfma.hpp"
#include "snn_conversion.hpp"

namespace snn {
namespace run_conv {

namespace cm = snn::conv_mfma;

constexpr int kStageRegs = 8;                    // band words of frame t + 1 a thread holds in registers while frame t is computed

__host__ __device__ __forceinline__ int slabs(const WideGeom &g) { return (int)((cm::padded_terms(g) + cm::kSlabRows - 1) / cm::kSlabRows); }
// bytes of the whole transposed bank of one channel group
__host__ __device__ __forceinline__ unsigned long long bank_bytes(const WideGeom &g) {
    return (unsigned long long)slabs(g) * cm::slab_floats(1) * sizeof(float);
}
__host__ __device__ __forceinline__ unsigned long long bands_bytes(const WideGeom &g) {
    const unsigned long long b = cm::band_bytes(g);
    return 2ull * (b < 16 ? 16 : b);
}
// whether the bank stays in LDS for all T: it must fit beside the two band buffers
__host__ __device__ __forceinline__ bool resident(const WideGeom &g) { return bank_bytes(g) + bands_bytes(g) <= (unsigned long long)cm::kLdsLimit; }
__host__ __device__ __forceinline__ unsigned long long lds_bytes(const WideGeom &g) {
    return (resident(g) ? bank_bytes(g) : 2ull * cm::slab_floats(1) * sizeof(float)) + bands_bytes(g);
}

// the band of the block of output pixels p0 .. p0 + kBlockPix - 1 of a sample
__host__ __device__ __forceinline__ cm::Band block_band(int p0, const WideGeom &g) { return cm::band_of(p0, (long)g.OH * g.OW, 0, g); }

// Word k of a band, in stage_band's order (consecutive k: consecutive pixels of one channel word): its value from the frame `sp`
// ([Cin, H * Wd] bytes), and its place among the slot's words.
__host__ __device__ __forceinline__ uint32_t band_word(const uint8_t *sp, const WideGeom &g, const cm::Band &band, int k) {
    const int npx = band.rows * g.Wd;
    return wide_stage_word(sp, g.Cin, g.H * g.Wd, band.iy0 * g.Wd + k % npx, k / npx);
}
__host__ __device__ __forceinline__ int band_word_slot(const WideGeom &g, const cm::Band &band, int k) {
    const int npx = band.rows * g.Wd;
    return (k % npx) * (wide_pixel_stride(g.Cin) / 4) + k / npx;
}
__host__ __device__ __forceinline__ int band_words(const WideGeom &g, const cm::Band &band) {
    return band.rows * g.Wd * (wide_pixel_stride(g.Cin) / 4);
}

// One neuron, one step, behind the convolution's sum `acc`: the current as snn_prop_conv2d_f32 stores it, the IF update, `summed`
// (where `sums`) and the trace `x` (read only where p.traces) as k_sif applies them.  Returns the spike byte.
__host__ __device__ __forceinline__ uint8_t current_step(float cur, float &v, float &rc, bool sums, float &summed, float &x,
                                                         const snn_lif_params &p) {
    const uint8_t sp = sif_update(v, rc, cur, p);
    if (p.traces) x = trace_next(x, sp, p.trace_decay, p.trace_scale, p.traces_additive);
    if (sums) summed = sif_summed(summed, cur);
    return sp;
}
__host__ __device__ __forceinline__ uint8_t neuron_step(float acc, const float *bias, int co, float &v, float &rc, bool sums, float &summed,
                                                        float &x, const snn_lif_params &p) {
    return current_step(wide_emit(acc, bias, co, 0.0f, 0), v, rc, sums, summed, x, p);
}

// One neuron over the Tc steps of a time chunk (snn_sif_scan): currents I[t * stride] as an operator left them, spike bytes to
// train[t * stride], the state in registers from step to step.  Returns the last step's spike.
__host__ __device__ __forceinline__ uint8_t scan_neuron(float &v, float &rc, bool sums, float &summed, float &x, const float *I, uint8_t *train,
                                                        int Tc, long stride, const snn_lif_params &p) {
    uint8_t sp = 0;
    for (int t = 0; t < Tc; ++t) {
        sp = current_step(I[(long)t * stride], v, rc, sums, summed, x, p);
        train[(long)t * stride] = sp;
    }
    return sp;
}

}  // namespace run_conv
}  // namespace snn
