// snn_run_dense_sif.hpp -- the order-carrying bodies of snn_run_dense_sif_f32 (csrc/snn_run_dense_sif.hip): a Connection over spike
// bytes and the SubtractiveResetIFNodes layer it feeds, over ALL T steps of a run in one launch (the layer-major plan of Network.run).
//
// Semantics, for t = 0 .. T-1, exactly the generic plan's: the current of step t is snn_prop_dense_auto_f32 of the source's frame of
// step t-1 (the start frame for t = 0) -- one unsplit f32 chain per (sample, target) over the sources ascending, the bias last, stored
// as 0 + sum (wide_emit, a lone feeder) --, then run_conv::current_step.  The GEMM is parallel in time: a tile of
// v_mfma_f32_16x16x4_f32 has 16 consecutive STEPS of one sample on its rows (row r reads the frame of step t0 + r - 1) and 16 targets
// on its columns, K = the sources in fours.  Why the bits agree is the argument of snn_conv_mfma.hpp and snn_mfma.hip: 1 * w and
// 0 * w are exact, the accumulator starts at +0 per tile and the current reaches `v` through sif_update only.  A block of steps whose
// staged rows hold a byte above 1 takes scalar_output below instead (one rounded multiply and one rounded add per non-zero byte, as
// the event-driven kernel).
//
// A workgroup owns ONE sample and a panel of kPanel = 64 targets for all T; wave w owns the panel's column tile w.  Time goes in super
// blocks of kSuper = 64 steps = kTimeBlocks independent accumulator tiles per wave, which share every weight operand.  LDS:
//   * the panel's weights in slabs of kSlabK sources, [source][kWStride] floats: an MFMA's B operand is 4 rows x 16 columns, and a
//     stride of 80 = 16 mod 64 starts the 4 rows 16 banks apart.  RESIDENT: every slab, staged during the first super block; else two
//     slabs that stream with every super block;
//   * two spike buffers [kSuper steps][kSpikeStride bytes] of kSlabK sources (+16: a row starts 4 banks after the one before).
// Epilogue: a lane holds rows (lane >> 4) * 4 + reg of column lane & 15.  The 16 lanes of group 0 step their four rows, then every
// lane takes (v, refrac, summed, x) from the lane 16 below it (handoff_source), group 1 steps, and so on round the wave: after the
// four groups of a time block the state is back in group 0 for the next block, in registers.
// The bodies are __host__ __device__: tests/hostcheck/run_dense_sif_host.hip drives them (tests/test_run_dense_sif_hostcheck.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "snn_common.hpp"
#include "snn_run_conv_sif.hpp"

namespace snn {
namespace run_dense {

namespace cm = snn::conv_mfma;
namespace da = snn::dense_auto;

constexpr int kTile = 16;                        // M, N of the MFMA
constexpr int kWaves = 4;
constexpr int kPanel = kTile * kWaves;           // targets per workgroup
constexpr int kTimeBlocks = 4;                   // accumulator tiles a wave keeps in flight
constexpr int kSuper = kTile * kTimeBlocks;      // steps per super block
constexpr int kSlabK = 64;                       // sources per slab: 4 rounds of four MFMAs per accumulator
constexpr int kWStride = kPanel + 16;            // floats per weight slab row
constexpr int kSpikeStride = kSlabK + 16;        // bytes per spike buffer row
constexpr int kSlabFloats = kSlabK * kWStride;
constexpr int kSpikeBytes = kSuper * kSpikeStride;

__host__ __device__ __forceinline__ int slabs(int Nin) { return (Nin + kSlabK - 1) / kSlabK; }
__host__ __device__ __forceinline__ unsigned long long panel_bytes(int Nin) { return (unsigned long long)slabs(Nin) * kSlabFloats * sizeof(float); }
// whether the panel stays in LDS for all T: it must fit beside the two spike buffers
__host__ __device__ __forceinline__ bool resident(int Nin) { return panel_bytes(Nin) + 2ull * kSpikeBytes <= (unsigned long long)cm::kLdsLimit; }
__host__ __device__ __forceinline__ unsigned long long lds_bytes(int Nin) {
    return (resident(Nin) ? panel_bytes(Nin) : 2ull * kSlabFloats * sizeof(float)) + 2ull * kSpikeBytes;
}

// the C layout of the 16x16 shapes: the step (row) and the target (column) of a lane's register
__host__ __device__ __forceinline__ int tile_row(int lane, int reg) { return (lane >> 4) * 4 + reg; }
__host__ __device__ __forceinline__ int tile_col(int lane) { return lane & 15; }
// the scan: phase ph = 0 .. 15 of a super block belongs to time block ph >> 2 and to the lanes of group ph & 3; behind every phase a
// lane takes the state of handoff_source(lane)
__host__ __device__ __forceinline__ int phase_group(int ph) { return ph & 3; }
__host__ __device__ __forceinline__ int handoff_source(int lane) { return (lane - 16) & 63; }

// the row of spike bytes that step t of sample b reads ([Nin] bytes): the start frame for t = 0, else frame t - 1 of the train
__host__ __device__ __forceinline__ const uint8_t *step_row(const uint8_t *s0, const uint8_t *s_train, int t, int b, int B, int Nin) {
    return t == 0 ? s0 + (size_t)b * Nin : s_train + ((size_t)(t - 1) * B + b) * Nin;
}
// sixteen bytes of that row from source kk on; a step at or beyond T and sources at or beyond Nin are zeros and are not read
__host__ __device__ __forceinline__ void stage_piece(const uint8_t *s0, const uint8_t *s_train, int t, int T, int b, int B, int Nin, int kk,
                                                     bool whole, uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (t < T) da::load_piece(step_row(s0, s_train, t, b, B, Nin), kk, Nin, whole, w);
}
// the weight at (source k, target col): 0 beyond Nin and beyond N; W [Nin, N]
__host__ __device__ __forceinline__ float panel_weight(const float *W, int Nin, int N, int k, int col) {
    const bool live = k < Nin && col < N;
    const float w = W[live ? (size_t)k * N + col : 0];                              // (always a valid address: no branch around the load)
    return live ? w : 0.0f;
}

// The scalar body: the sum of (row, target col) in the stated order -- zero bytes skipped, one rounded multiply and one rounded add per
// other byte (-ffp-contract=off): dense_auto::chain_mul_add down a column of W.  Slow and exact for any byte.
__host__ __device__ __forceinline__ float scalar_output(const uint8_t *row, const float *W, int Nin, int N, int col) {
    float acc = 0.0f;
    for (int k = 0; k < Nin; ++k) {
        const uint8_t sv = row[k];
        if (!sv) continue;
        const float t = W[(size_t)k * N + col] * (float)sv;
        acc = acc + t;
    }
    return acc;
}

// A lane's turn in the scan: its four rows of time block t0 (steps t0 + tile_row(lane, reg)) of target col of sample b, from the sums
// acc[4]; steps at or beyond T change nothing.  Spike bytes go to out_train [T, B, N], the last step's to s [B, N] too.
__host__ __device__ __forceinline__ void scan_rows(const float (&acc)[4], int lane, int t0, int T, int b, int B, int N, int col, const float *bias,
                                                   float &v, float &rc, bool sums, float &summed, float &x, const snn_lif_params &p,
                                                   uint8_t *out_train, uint8_t *s) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int t = t0 + tile_row(lane, reg);
        if (t >= T) break;
        const uint8_t sp = run_conv::neuron_step(acc[reg], bias, col, v, rc, sums, summed, x, p);
        out_train[((size_t)t * B + b) * N + col] = sp;
        if (t == T - 1) s[(size_t)b * N + col] = sp;
    }
}

}  // namespace run_dense
}  // namespace snn
