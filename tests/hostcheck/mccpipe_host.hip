// Host-side check of the feature-pipeline kernels' arithmetic (bindsnet_amd/csrc/snn_mccpipe.hpp: the per-synapse term program,
// the draw-to-bit conversion, the bit-mask layout) driven by the ordered-sum accumulators of csrc/snn_order.hpp exactly as the
// threads of k_prop_mcc_pipe / k_mcc_bernoulli drive them, and compared with torch by tests/test_mcc_pipe_hostcheck.py.
// Compiled by hipcc like the kernels (same front end, -ffp-contract=off); no device code is executed.  Test infrastructure only.
#include <stdint.h>
#include "../../bindsnet_amd/csrc/snn_mccpipe.hpp"
#include "../../bindsnet_amd/csrc/snn_order.hpp"

using namespace snn;

// k_prop_mcc_pipe's thread (sample b, column j).  val[k]: f32 [S, N] (MUL_F32 / ADD_F32), u8 [S, N] (MUL_MASK) or the uint32
// bit mask (MUL_DRAW); scalar[k]: one element.  Without an ADD op silent rows are skipped, as on the device.
extern "C" void hostcheck_mcc_prop(int n_ops, const int *kind, const void *const *val, const int *scalar, const uint8_t *s, int B, int Nin,
                                   int N, float *out) {
    bool has_add = false;
    for (int k = 0; k < n_ops; ++k) has_add = has_add || kind[k] == SNN_MCC_OP_ADD_F32;
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < N; ++j) {
            const uint8_t *srow = s + (size_t)b * Nin;
            OuterSum acc;
            acc.init(j >= (N / 32) * 32);
            for (int i = 0; i < Nin; ++i) {
                if (!has_add && !srow[i]) continue;
                const float term = mcc_term((float)srow[i], n_ops, kind, [&](int k) -> float {
                    const size_t at = scalar[k] ? 0 : (size_t)i * N + j;
                    if (kind[k] == SNN_MCC_OP_MUL_DRAW) return mcc_bit_operand((const uint32_t *)val[k], i, j, N);
                    if (kind[k] == SNN_MCC_OP_MUL_MASK) return (float)(((const uint8_t *)val[k])[at] != 0);
                    return ((const float *)val[k])[at];
                });
                acc.add(i, term, Nin);
            }
            out[(size_t)b * N + j] = 0.0f + acc.finish(Nin);
        }
}

// k_mcc_bernoulli, serially: S*N outputs of at::mt19937 from a 624-word state image and the index of its next output (624 = twist
// first) -> bits [S, ceil(N/32)]; the state is advanced in place, *pos updated.
extern "C" void hostcheck_mcc_bernoulli(uint32_t *mt, int *pos, const float *p, int p_scalar, int S, int N, uint32_t *bits) {
    uint32_t nxt[624];
    int q = *pos;
    const int nw = mcc_bit_words(N);
    for (long k = 0; k < (long)S * nw; ++k) bits[k] = 0u;
    for (int i = 0; i < S; ++i)
        for (int j = 0; j < N; ++j) {
            if (q >= 624) {                                          // the twist of mt_twist_block, serially
                for (int a = 0; a < 227; ++a) nxt[a] = mt[a + 397] ^ mt_mix(mt[a], mt[a + 1]);
                for (int a = 227; a < 454; ++a) nxt[a] = nxt[a - 227] ^ mt_mix(mt[a], mt[a + 1]);
                for (int a = 454; a < 624; ++a) nxt[a] = nxt[a - 227] ^ mt_mix(mt[a], a == 623 ? nxt[0] : mt[a + 1]);
                for (int a = 0; a < 624; ++a) mt[a] = nxt[a];
                q = 0;
            }
            if (mcc_draw_hit(mt[q++], p_scalar ? p[0] : p[(size_t)i * N + j])) bits[(size_t)i * nw + (j >> 5)] |= 1u << (j & 31);
        }
    *pos = q;
}
