// snn_normstep.hpp -- Weight(norm_frequency="time step"): one column tile of snn_prop_cascade_norm_f32, as __host__ __device__ text.
//
// The reference's Weight.compute (topology_features.py:633-645) forms value * conn_spikes and then normalises the value in place
// (AbstractFeature.normalize, :250-266): the step's currents come from the OLD weights, the next step reads the scaled ones.  The
// fused kernel (snn_normstep.hip) gives a workgroup kPnCols columns of W with all their rows in LDS; everything it computes from that
// tile is one of the functions below, so tests/hostcheck/norm_step_host.hip runs the same text on the CPU, tile by tile, against torch
// (tests/test_norm_step_hostcheck.py).  The arithmetic is that of k_prop (currents) and of colsum_body / k_scale_cols (normalisation)
// in snn_ops.hip -- the contract is bit identity with snn_prop_cascade_f32 followed by snn_normalize / snn_normalize_pv (use_abs 0).
//
// ATen's sum(dim=0) of one column of N >= 2 (snn_order.hpp): a cascade column is ONE sequence of its Nin terms, a row_sum column FOUR
// (rows 4p + q, p < Nin / 4) and the Nin % 4 leftover rows.  A sequence is a cascade over 16-term blocks: the block sums are
// independent of each other (pn_block_sum, one thread each), only folding them is sequential (pn_seq_fold, one thread per sequence).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "snn_order.hpp"
#include "snn_synparams.hpp"

namespace snn {

constexpr int kPnCols = 16;       // columns of a tile (tile[i * kPnCols + c] = W[i, j0 + c])
constexpr int kPnSamples = 16;    // samples of one pass: 256 threads = kPnSamples x kPnCols (sample, column) pairs
constexpr int kPnThreads = kPnCols * kPnSamples;

__host__ __device__ __forceinline__ int pn_seq_len(bool tail, int Nin) { return tail ? Nin >> 2 : Nin; }
// block sums a column keeps: the cascade's Nin / 16, or row_sum's 4 * (Nin / 64) <= Nin / 16, interleaved by sequence
__host__ __device__ __forceinline__ int pn_blocks_per_col(int Nin) { return Nin >> 4; }
__host__ __device__ __forceinline__ int pn_block_items(bool tail, int Nin) { return tail ? 4 * ((Nin >> 2) >> 4) : Nin >> 4; }

// term p of sequence q of tile column c
__host__ __device__ __forceinline__ float pn_term(const float *tile, int c, bool tail, int q, int p) {
    return tile[(size_t)(tail ? 4 * p + q : p) * kPnCols + c];
}

// item r of a column's block sums: block r of the cascade, or block r / 4 of row_sum's sequence r % 4
__host__ __device__ __forceinline__ float pn_block_sum(const float *tile, int c, bool tail, int r) {
    const int q = tail ? r & 3 : 0, blk = tail ? r >> 2 : r;
    float a0 = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) a0 += pn_term(tile, c, tail, q, blk * 16 + k);
    return a0;
}

// sequence q of column c from the column's block sums `bs`: the upper cascade levels in block order, then the terms past the last
// complete block (colsum_body's fold, snn_ops.hip)
__host__ __device__ __forceinline__ float pn_seq_fold(const float *bs, const float *tile, int c, bool tail, int q, int Nin) {
    const int n = pn_seq_len(tail, Nin), nfull = n >> 4, stride = tail ? 4 : 1;
    float a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int b2 = 0; b2 < nfull; ++b2) {
        a1 += bs[b2 * stride + q];
        const int m = b2 + 1;
        if ((m & 15) == 0) { a2 += a1; a1 = 0.f; if ((m & 255) == 0) { a3 += a2; a2 = 0.f; } }
    }
    float a0 = 0.f;
    for (int p = nfull * 16; p < n; ++p) a0 += pn_term(tile, c, tail, q, p);
    return ((a0 + a1) + a2) + a3;
}

// the column's sum from its sequences' sums: the Nin % 4 leftover rows join lane 0 behind its cascade, then ((l0 + l1) + l2) + l3
__host__ __device__ __forceinline__ float pn_colsum(const float *seq, const float *tile, int c, bool tail, int Nin) {
    if (!tail) return seq[0];
    float l0 = seq[0];
    for (int i = (Nin >> 2) * 4; i < Nin; ++i) l0 += tile[(size_t)i * kPnCols + c];
    return ((l0 + seq[1]) + seq[2]) + seq[3];
}

// topology_features.py:264-266: a zero sum becomes 1; a python-float norm is ATen's reciprocal-then-multiply (snn_normalize), a
// tensor norm one IEEE division (snn_normalize_pv: syn_norm_scale)
__host__ __device__ __forceinline__ float pn_scale(float cs, float norm) {
    if (cs == 0.f) cs = 1.0f;
    return (1.0f / cs) * norm;
}
__host__ __device__ __forceinline__ float pn_scale_pv(float cs, float norm_j) { return syn_norm_scale(norm_j, cs); }

// out[b, j]'s sum over the sample's spiking sources, ascending (k_prop's walk): list entries are (i << 8) | s[b, i]
__host__ __device__ __forceinline__ float pn_current(const float *tile, int c, const uint32_t *list, int cnt, int Nin, bool tail) {
    OuterSum acc;
    acc.init(tail);
    for (int k = 0; k < cnt; ++k) {
        const uint32_t e = list[k];
        acc.add((int)(e >> 8), tile[(size_t)(e >> 8) * kPnCols + c] * (float)(e & 255u), Nin);
    }
    return acc.finish(Nin);
}

// ONE target column (N == 1): the sums over the sources are ATen's inner reduction (k_prop_col1 / k_colsum_few)
__host__ __device__ inline float pn_col1_current(const float *W, const uint8_t *srow, int Nin) {
    return inner_sum8_terms([=](int i) { return W[i] * (float)srow[i]; }, Nin);
}
__host__ __device__ inline float pn_col1_sum(const float *W, int Nin) {
    return inner_sum8_terms([=](int i) { return W[i]; }, Nin);
}

// LDS of one workgroup, in bytes: the tile, its block sums, the sequences' sums and the scales, the spike lists and their counts
__host__ __device__ inline size_t pn_lds_bytes(int Nin) {
    return sizeof(float) * ((size_t)Nin * kPnCols + (size_t)(pn_blocks_per_col(Nin) + 1) * kPnCols + 4 * kPnCols + kPnCols) +
           sizeof(uint32_t) * ((size_t)kPnSamples * Nin + kPnSamples);
}

}  // namespace snn
