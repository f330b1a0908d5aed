// snn_mccpipe.hpp -- what one synapse of a MulticompartmentConnection feature pipeline computes, and how a draw becomes a bit.
//
// The reference (bindsnet/network/topology.py:437-479) repeats the spikes into conn_spikes [B, S, N], hands them to every
// feature's compute() in list order (topology_features.py: Probability x * bernoulli(value), Mask x * value, Weight value * x,
// Bias x + value, Intensity x * value) and reduces with conn_spikes.sum(1).  Per (b, i, j) that is a short program of f32
// multiplies and adds on float(s[b,i]); a Bernoulli outcome and a mask entry enter as the factors 1.0f / 0.0f, exactly as torch
// multiplies by them, so signed zeros and non-finite values come out as they do there.  Built with -ffp-contract=off: every
// operation below is one rounding.  The functions are __host__ __device__: tests/hostcheck/mccpipe_host.hip runs them on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_rng.hpp"

namespace snn {

// One op of the program applied to the running term t; `operand` is the synapse's value (0.0f / 1.0f for a draw or a mask entry).
__host__ __device__ __forceinline__ float mcc_apply(float t, int kind, float operand) {
    return kind == SNN_MCC_OP_ADD_F32 ? t + operand : t * operand;
}

// The whole program on one synapse: starts at float(s[b,i]), ops in pipeline order; operand(k) yields op k's value there.
template <class OPERAND>
__host__ __device__ __forceinline__ float mcc_term(float s, int n_ops, const int *kind, OPERAND operand) {
    float t = s;
    for (int k = 0; k < n_ops; ++k) t = mcc_apply(t, kind[k], operand(k));
    return t;
}

// torch.bernoulli(p) on the CPU generator, one element: ONE raw mt19937 state word y -> tempered r -> u = (r & 0xFFFFFF) * 2^-24
// (exact in f32) -> u < p.  The same conversion as k_encode_bernoulli (csrc/snn_encode.hip).
__host__ __device__ __forceinline__ bool mcc_draw_hit(uint32_t y, float p) {
    const uint32_t r = mt_temper(y);
    const float u = (float)(r & 0xFFFFFFu) * 5.9604644775390625e-08f;
    return u < p;
}

// Where element (i, j) of an [S, N] draw lives in the bit-packed [S, ceil(N / 32)] mask: rows start on word boundaries.
__host__ __device__ __forceinline__ int mcc_bit_words(int N) { return (N + 31) >> 5; }
__host__ __device__ __forceinline__ float mcc_bit_operand(const uint32_t *bits, int i, int j, int N) {
    return (float)((bits[(size_t)i * mcc_bit_words(N) + (j >> 5)] >> (j & 31)) & 1u);
}

}  // namespace snn
