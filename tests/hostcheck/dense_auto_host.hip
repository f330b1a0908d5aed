// Host-side check of bindsnet_amd/csrc/snn_dense_auto.hpp: the __host__ __device__ text that snn_prop_dense_auto_f32's kernels decide
// with -- the census of a tile's spike bytes, the cost rule, and the two accumulator chains whose equality for 0/1 factors is why the
// bodies agree -- is run HERE on the CPU (compiled by hipcc like the kernels, no device code is executed).  Test infrastructure only
// (tests/test_dense_auto_hostcheck.py); not part of libsnnhip.
#include <stdint.h>
#include <string.h>
#include "../../bindsnet_amd/csrc/snn_dense_auto.hpp"

using namespace snn::dense_auto;

// out[tile] = {largest count of a valid row, any byte above 1} for every tile of 16 samples of s [B, Nin]
extern "C" int hostcheck_census(const uint8_t *s, int B, int Nin, int *out) {
    if (!s || !out || B <= 0 || Nin <= 0) return -1;
    for (int t = 0; t * kTile < B; ++t) {
        const census c = census_tile(s, B, Nin, t * kTile);
        out[2 * t] = c.count;
        out[2 * t + 1] = c.above1;
    }
    return 0;
}

extern "C" int hostcheck_use_matrix(int max_count, int above1, int rows, int Nin, int N, int B, int mode) {
    return use_matrix(max_count, above1, rows, Nin, N, B, mode);
}

// the bit patterns of the two chains over n (byte, weight) pairs
extern "C" void hostcheck_chains(const uint8_t *byte, const float *w, int n, uint32_t *fma_bits, uint32_t *mul_add_bits) {
    const float a = chain_fma(byte, w, n), b = chain_mul_add(byte, w, n);
    memcpy(fma_bits, &a, 4);
    memcpy(mul_add_bits, &b, 4);
}
