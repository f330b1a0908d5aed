// Host-side check of bindsnet_amd/csrc/snn_normstep.hpp: the __host__ __device__ text of snn_prop_cascade_norm(_pv)_f32 is run HERE on
// the CPU (compiled by hipcc like the kernels, no device code is executed), tile by tile and work item by work item as the threads
// of k_prop_norm / k_prop_norm_col1 (csrc/snn_normstep.hip) run it: the tile is copied out of W, its block sums, sequence sums, column
// sums and scales are formed, every sample's ascending spike list is walked, and the tile goes back scaled.  Test infrastructure
// only (tests/test_norm_step_hostcheck.py); not part of libsnnhip.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_normstep.hpp"

using namespace snn;

// norm_vec NULL: the scalar `norm`.  Returns the LDS bytes the device tile would need (the caller checks the limit), < 0 on error.
extern "C" long hostcheck_prop_norm(float *W, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate, float norm,
                                    const float *norm_vec) {
    if (!W || !s || !out || B <= 0 || Nin <= 0 || N <= 0 || Nin > kMaxTerms) return -1;
    if (N == 1) {                                             // k_prop_norm_col1
        for (int b = 0; b < B; ++b) {
            const float r = pn_col1_current(W, s + (size_t)b * Nin, Nin);
            out[b] = (accumulate ? out[b] : 0.0f) + r;
        }
        const float cs = pn_col1_sum(W, Nin);
        const float sc = norm_vec ? pn_scale_pv(cs, norm_vec[0]) : pn_scale(cs, norm);
        for (int i = 0; i < Nin; ++i) W[i] = W[i] * sc;
        return 0;
    }
    const int nbs = pn_blocks_per_col(Nin) + 1;
    std::vector<float> tile((size_t)Nin * kPnCols), bs((size_t)nbs * kPnCols), seq(4 * kPnCols), scale(kPnCols);
    std::vector<uint32_t> list((size_t)Nin);
    for (int j0 = 0; j0 < N; j0 += kPnCols) {                 // one workgroup
        for (int idx = 0; idx < Nin * kPnCols; ++idx) {
            const int i = idx / kPnCols, j = j0 + idx % kPnCols;
            tile[idx] = W[(size_t)i * N + (j < N ? j : N - 1)];
        }
        for (int it = 0; it < (Nin >> 4) * kPnCols; ++it) {
            const int c = it % kPnCols, r = it / kPnCols;
            const bool tail = outer_tail(j0 + c, N);
            if (r < pn_block_items(tail, Nin)) bs[c * nbs + r] = pn_block_sum(tile.data(), c, tail, r);
        }
        for (int t = 0; t < 4 * kPnCols; ++t) {
            const int c = t % kPnCols, q = t / kPnCols;
            const bool tail = outer_tail(j0 + c, N);
            if (tail || q == 0) seq[c * 4 + q] = pn_seq_fold(bs.data() + c * nbs, tile.data(), c, tail, q, Nin);
        }
        for (int c = 0; c < kPnCols; ++c) {
            const int j = j0 + c;
            const float cs = pn_colsum(seq.data() + c * 4, tile.data(), c, outer_tail(j, N), Nin);
            scale[c] = norm_vec ? pn_scale_pv(cs, norm_vec[j < N ? j : N - 1]) : pn_scale(cs, norm);
        }
        for (int b = 0; b < B; ++b) {
            int n = 0;                                        // the wave's ballot compaction: the spiking sources, ascending
            for (int i = 0; i < Nin; ++i)
                if (s[(size_t)b * Nin + i]) list[n++] = ((uint32_t)i << 8) | s[(size_t)b * Nin + i];
            for (int c = 0; c < kPnCols && j0 + c < N; ++c) {
                const float r = pn_current(tile.data(), c, list.data(), n, Nin, outer_tail(j0 + c, N));
                const size_t o = (size_t)b * N + j0 + c;
                out[o] = (accumulate ? out[o] : 0.0f) + r;
            }
        }
        for (int idx = 0; idx < Nin * kPnCols; ++idx) {
            const int i = idx / kPnCols, c = idx % kPnCols;
            if (j0 + c < N) W[(size_t)i * N + j0 + c] = tile[idx] * scale[c];
        }
    }
    return (long)pn_lds_bytes(Nin);
}
