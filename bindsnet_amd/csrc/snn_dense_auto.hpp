// snn_dense_auto.hpp -- what snn_prop_dense_auto_f32 (csrc/snn_mfma.hip) decides with, as __host__ __device__ text: the census of a
// 16-sample tile's spike bytes and the cost rule that picks the tile's body.  The kernels use these functions;
// tests/hostcheck/dense_auto_host.hip compiles the same text for the host and drives it (tests/test_dense_auto_hostcheck.py).
//
// Why the two bodies agree: the event-driven kernel adds `w * (float)byte` to its chain, a rounded multiply and a rounded add; the
// f32 MFMA adds fma(byte, w, acc), one rounding.  For a byte of 0 or 1 the product is exact (w, or a zero whose sign cannot turn a
// chain that started at +0 into -0), so both are the same rounded add -- chain_fma and chain_mul_add below, which the host check
// compares over signed, subnormal and zero weights.  For another byte they differ, so a tile that holds one takes the event body.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>


namespace snn {
namespace dense_auto {

constexpr int kTile = 16;               // samples per tile: the M of v_mfma_f32_16x16x4_f32
constexpr int kPiece = 16;              // spike bytes per census piece: one 16-byte load

// snn_set_dense_prop_mode
constexpr int kModeRule = 0, kModeEvent = 1, kModeMatrix = 2;

// ---- the cost rule's constants -----------------------------------------------------------------------------------------------
// Measured on one MI355X by tools/bench_dense_auto.py; every window is in profiles/NOTES_dense_auto.md, the numbers these were
// fitted to in profiles/dense_auto_calibration.jsonl.  All in nanoseconds.  A wrong value costs time, never bits.
constexpr int kEventNs = 100;           // one more entry in the event list of the tile's busiest row: 75 .. 100 ns at 16 samples (the walk is
                                        //  latency-bound: a dependent pass over 1 KiB row segments of W)
constexpr int kRoundNs = 130;           // one more round of the chain, 16 sources: (60.7 - 12.4) us over the 351 rounds between 784 and 6400 sources
constexpr int kMatrixFixedNs = 1500;    // puts the crossing at 6400 sources where it was measured (505 .. 545 events against 400 rounds)
// Both kernels put four waves in a workgroup; the event-driven one has ceil(N / 256) workgroups per SAMPLE, the matrix one
// ceil(N / 64) per TILE.  Up to this many waves a launch costs what one workgroup costs; beyond, in proportion (an event costs twice
// as much at 128 x 784 -> 1600, 3584 waves, as at 16 samples).
constexpr int kResidentWaves = 2048;

// snn_net_run hands a connection to snn_prop_dense_auto_f32 under the rule only if its owner asked for it (snn_conn_prop.prop_auto)
// AND it has this many sources: the second launch costs every step 3 to 6 us whatever the spikes are (profiles/NOTES_dense_auto.md:
// the breakout graph at 1 % input density lost 6.5 % of its step to it), so a graph that never asked keeps the single event-driven launch
// and its speed, and fewer sources cannot win the launch back even when dense (256 -> 128 loses 4 us up to 20 % density and gains
// from 50 % on, 100 -> 4 only loses).  Modes 1 and 2 -- tests, measurements -- take every connection that has a table entry.
constexpr int kMinSources = 256;
__host__ __device__ inline bool worth_a_launch(int Nin, int asked, int mode) { return mode != kModeRule || (asked && Nin >= kMinSources); }

struct census {
    int count;                          // non-zero bytes
    int above1;                         // != 0: a byte that is neither 0 nor 1
};

struct alignas(16) piece16 { uint32_t w[4]; };

// the census of four spike bytes in a word
__host__ __device__ inline void census_word(uint32_t w, census &c) {
    uint32_t t = w | (w >> 1);          // bit 0 of every byte <- the OR of its eight bits (what leaks in from the byte above lands in bits 1 .. 7 only)
    t |= t >> 2;
    t |= t >> 4;
    c.count += __builtin_popcount(t & 0x01010101u);
    c.above1 |= (int)((w & 0xFEFEFEFEu) != 0u);
}

// sixteen spike bytes of a row, sources kk .. kk + 15, as four little-endian words; sources at and beyond Nin are zeros.  `whole`: the
// row length is a multiple of 16 and the row starts 16-byte aligned, so the piece is one aligned 16-byte load (the kernel's fast path)
__host__ __device__ inline void load_piece(const uint8_t *row, int kk, int Nin, bool whole, uint32_t (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (kk >= Nin) return;
    if (whole) {
        const piece16 p = *(const piece16 *)(row + kk);
        w[0] = p.w[0]; w[1] = p.w[1]; w[2] = p.w[2]; w[3] = p.w[3];
        return;
    }
    for (int u = 0; u < kPiece; ++u)
        if (kk + u < Nin) w[u >> 2] |= (uint32_t)row[kk + u] << (8 * (u & 3));
}

__host__ __device__ inline void census_piece(const uint32_t (&w)[4], census &c) {
    census_word(w[0], c); census_word(w[1], c); census_word(w[2], c); census_word(w[3], c);
}

// what a tile's workgroups reduce their rows' censuses to: the largest count of a valid row, the OR of the rows' above1
__host__ __device__ inline void census_merge(census &tile, const census &row) {
    tile.count = row.count > tile.count ? row.count : tile.count;
    tile.above1 |= row.above1;
}

// the census of the tile of samples m0 .. m0 + 15 of s [B, Nin], piece by piece as the kernel's threads walk it; rows at and beyond B
// do not exist and count nothing
__host__ __device__ inline census census_tile(const uint8_t *s, int B, int Nin, int m0) {
    census tile = {0, 0};
    const bool whole = (Nin & 15) == 0 && ((uintptr_t)s & 15) == 0;
    for (int r = 0; r < kTile && m0 + r < B; ++r) {
        census row = {0, 0};
        for (int kk = 0; kk < Nin; kk += kPiece) {
            uint32_t w[4];
            load_piece(s + (size_t)(m0 + r) * Nin, kk, Nin, whole, w);
            census_piece(w, row);
        }
        census_merge(tile, row);
    }
    return tile;
}

// The rule: 1 = the tile takes the matrix body.  max_count: the largest event count among the tile's `rows` valid rows.
// Never 1 with a byte above 1 (the bits would differ) and never for a silent tile (the event body then only writes the bias).
// Mode 0: matrix if the walk of the longest event list costs more than Nin / 16 rounds of the chain.  Integer arithmetic, so that
// every workgroup of a tile, and the host, reach the same answer.
__host__ __device__ inline int use_matrix(int max_count, int above1, int rows, int Nin, int N, int B, int mode) {
    if (above1 || rows <= 0 || max_count <= 0 || mode == kModeEvent) return 0;
    if (mode == kModeMatrix) return 1;
    const long long rounds = (Nin + 15) >> 4;
    const long long ev_waves = 4ll * B * ((N + 255) >> 8), mx_waves = 4ll * ((B + kTile - 1) / kTile) * ((N + 63) >> 6);
    // (x kResidentWaves on both sides instead of a divide: a launch that fits the machine costs one workgroup's time)
    const long long cap = 1ll << 30;    // (keeps the products below inside 63 bits for any Nin < 2^24)
    const long long ev_scale = ev_waves > cap ? cap : ev_waves > kResidentWaves ? ev_waves : kResidentWaves;
    const long long mx_scale = mx_waves > cap ? cap : mx_waves > kResidentWaves ? mx_waves : kResidentWaves;
    const long long event_cost = (long long)max_count * kEventNs * ev_scale;
    const long long matrix_cost = (rounds * kRoundNs + kMatrixFixedNs) * mx_scale;
    return event_cost > matrix_cost ? 1 : 0;
}

// ---- the two chains, for the host check: acc over k of byte[k] and w[k] -------------------------------------------------------------
__host__ __device__ inline float chain_fma(const uint8_t *byte, const float *w, int n) {         // the MFMA: one rounding per term
    float a = 0.f;
    for (int k = 0; k < n; ++k) a = __builtin_fmaf((float)byte[k], w[k], a);
    return a;
}
__host__ __device__ inline float chain_mul_add(const uint8_t *byte, const float *w, int n) {     // k_prop: zero bytes skipped, product and sum rounded
    float a = 0.f;
    for (int k = 0; k < n; ++k)
        if (byte[k]) { const float p = w[k] * (float)byte[k]; a = a + p; }
    return a;
}

}  // namespace dense_auto
}  // namespace snn
