// snn_mccpipe.hip -- MulticompartmentConnection feature pipelines on the MI355X (bindsnet/network/topology.py:437-479,
// bindsnet/network/topology_features.py: Probability / Mask / Weight / Bias / Intensity).
//
//  * snn_mcc_bernoulli: the mask torch.bernoulli(value) draws for ONE compute() call of a Probability feature, bit-packed.
//    S*N consecutive 32-bit outputs of the HOST generator, row-major, u = (r & 0xFFFFFF) * 2^-24 < p -- the stream of
//    snn_encode_bernoulli.  mt19937 has no cheap jump-ahead: one workgroup walks the stream, twisting a 624-word block
//    cooperatively and turning it into 624 bits; the partially consumed block stays in *rng for whoever draws next.
//  * snn_prop_mcc_pipe_f32: out[b,j] (+)= sum_i term(b,i,j), term = the feature program of csrc/snn_mccpipe.hpp on
//    float(s[b,i]), summed in ATen's sum(dim=1) order with the accumulators of csrc/snn_order.hpp, as snn_prop_cascade_f32.
//    Without an additive op a silent source row contributes +-0 to every column (values are finite) and is skipped, its
//    flush boundaries kept by the accumulators; with one (Bias) every row is a term and the walk is dense.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_mccpipe.hpp"
#include "snn_order.hpp"
#include "snn_rng.hpp"

namespace {
using namespace snn;

constexpr int BNT = 256;            // 4 waves: a 227-word twist stripe is one pass, and the three barriers of a twist stay cheap

// p_scalar: p[0] for every synapse.  bits must be zeroed: a word shared by two 624-blocks or two waves is completed by both.
__global__ __launch_bounds__(BNT) void k_mcc_bernoulli(snn_rng_state *rng, const float *__restrict__ p, int p_scalar, int S, int N,
                                                        uint32_t *bits) {
    __shared__ uint32_t mt[2][624];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < 624; k += BNT) mt[0][k] = rng->mt[k];
    int pos = rng->pos, cur = 0;
    __syncthreads();
    const long long total = (long long)S * N;
    const int nw = mcc_bit_words(N);
    long long e = 0;
    while (e < total) {
        // (no barrier in front of the twist: it reads mt[cur], which the conversion below only reads, and writes the buffer whose
        //  last readers passed the three barriers of the previous twist)
        if (pos >= 624) { mt_twist_block(mt[cur], mt[cur ^ 1], tid, BNT); cur ^= 1; pos = 0; }
        const int avail = (int)((long long)(624 - pos) < total - e ? (long long)(624 - pos) : total - e);
        const int i0 = (int)(e / N), j0 = (int)(e - (long long)i0 * N);      // (one 64-bit division per block, uniform)
        for (int k0 = 0; k0 < avail; k0 += BNT) {          // whole waves enter: the ballot needs every lane
            const int k = k0 + tid;
            const bool live = k < avail;
            const unsigned jj = (unsigned)j0 + (unsigned)(live ? k : 0), di = jj / (unsigned)N;      // < N + 624: fits 32 bits
            const int i = i0 + (int)di, j = (int)(jj - di * (unsigned)N);
            const bool hit = live && mcc_draw_hit(mt[cur][pos + (live ? k : 0)], p_scalar ? p[0] : p[(size_t)i * N + j]);
            const unsigned long long m = __ballot(hit);
            // consecutive lanes are consecutive bits of one word until the word or the row ends (rows start on word boundaries):
            // the first lane of every such run ORs the run's bits in
            const int bit = j & 31;
            const bool lead = live && (lane == 0 || bit == 0);
            if (lead) {
                int run = 32 - bit;
                if (run > N - j) run = N - j;
                if (run > 64 - lane) run = 64 - lane;
                const uint32_t v = (uint32_t)((m >> lane) & ((1ull << run) - 1ull)) << bit;      // (lanes past `avail` voted 0)
                if (v) atomicOr(&bits[(size_t)i * nw + (j >> 5)], v);
            }
        }
        pos += avail; e += avail;
    }
    __syncthreads();
    for (int k = tid; k < 624; k += BNT) rng->mt[k] = mt[cur][k];
    if (tid == 0) rng->pos = pos;
}

struct PipeProg {
    int n, has_add;
    int kind[SNN_MCC_MAX_PIPE], scalar[SNN_MCC_MAX_PIPE];
    const void *val[SNN_MCC_MAX_PIPE];
    const uint32_t *bits[SNN_MCC_MAX_PIPE];
};

// The operands of synapse (i, j) and the term they give.
__device__ __forceinline__ float pipe_term(const PipeProg &P, float sv, int i, int j, int N) {
    return mcc_term(sv, P.n, P.kind, [&](int k) -> float {
        const size_t at = P.scalar[k] ? 0 : (size_t)i * N + j;
        if (P.kind[k] == SNN_MCC_OP_MUL_DRAW) return mcc_bit_operand(P.bits[k], i, j, N);
        if (P.kind[k] == SNN_MCC_OP_MUL_MASK) return (float)(((const uint8_t *)P.val[k])[at] != 0);
        return ((const float *)P.val[k])[at];
    });
}

// grid (ceil(N/256), B), 256 threads: thread <-> target column j, block <-> sample b, as k_prop (csrc/snn_ops.hip).
__global__ __launch_bounds__(256) void k_prop_mcc_pipe(PipeProg P, const uint8_t *__restrict__ s, float *__restrict__ out, int B,
                                                       int Nin, int N, int accumulate) {
    __shared__ uint32_t list[4][256];
    __shared__ int cnt[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y, j = blockIdx.x * 256 + tid;
    const bool valid = j < N;
    const int jc = valid ? j : N - 1;
    const uint8_t *srow = s + (size_t)b * Nin;
    OuterSum acc;
    acc.init(outer_tail(j, N));
    if (P.has_add) {                       // every row is a term: the dense walk, same positions, same flush boundaries
        for (int i = 0; i < Nin; ++i) acc.add(i, pipe_term(P, (float)srow[i], i, jc, N), Nin);
    } else {
        const uint64_t lt = (1ull << lane) - 1ull;
        for (int base = 0; base < Nin; base += 1024) {
            int n_w = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int i = base + wave * 256 + p * 64 + lane;
                const uint32_t sv = (i < Nin) ? srow[i] : 0u;
                const uint64_t m = __ballot(sv != 0);
                if (sv) list[wave][n_w + __popcll(m & lt)] = ((uint32_t)i << 8) | sv;
                n_w += __popcll(m);
            }
            if (lane == 0) cnt[wave] = n_w;
            __syncthreads();
            for (int w = 0; w < 4; ++w) {
                const int n = cnt[w];
                for (int k = 0; k < n; ++k) {
                    const uint32_t e = list[w][k];
                    const int i = (int)(e >> 8);
                    acc.add(i, pipe_term(P, (float)(e & 255u), i, jc, N), Nin);
                }
            }
            __syncthreads();
        }
    }
    if (valid) {
        const float r = acc.finish(Nin);
        const size_t o = (size_t)b * N + j;
        out[o] = (accumulate ? out[o] : 0.0f) + r;
    }
}

}  // namespace

extern "C" int snn_mcc_bernoulli(snn_rng_state *rng, const float *p, int p_scalar, int S, int N, uint32_t *bits, snn_stream_t stream) {
    if (!rng || !p || !bits || S <= 0 || N <= 0) return SNN_ERR_INVALID;
    if ((long long)S * mcc_bit_words(N) > (1ll << 31) - 1) return SNN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (snn_check(hipMemsetAsync(bits, 0, sizeof(uint32_t) * (size_t)S * mcc_bit_words(N), st))) return SNN_ERR_LAUNCH;
    hipLaunchKernelGGL(k_mcc_bernoulli, dim3(1), dim3(BNT), 0, st, rng, p, p_scalar, S, N, bits);
    return snn_check_launch();
}

extern "C" int snn_prop_mcc_pipe_f32(const snn_mcc_op *h_ops, int n_ops, const uint8_t *s, float *out, int B, int Nin, int N,
                                     int accumulate, snn_stream_t stream) {
    if (!h_ops || !s || !out || B <= 0 || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (n_ops <= 0 || n_ops > SNN_MCC_MAX_PIPE) return SNN_ERR_INVALID;
    if (Nin > kMaxTerms || B > 65535) return SNN_ERR_UNSUPPORTED;
    PipeProg P = {};
    P.n = n_ops;
    for (int k = 0; k < n_ops; ++k) {
        const snn_mcc_op &o = h_ops[k];
        if (o.kind < SNN_MCC_OP_MUL_DRAW || o.kind > SNN_MCC_OP_ADD_F32) return SNN_ERR_INVALID;
        if (o.kind == SNN_MCC_OP_MUL_DRAW ? !o.bits : !o.val) return SNN_ERR_INVALID;
        P.kind[k] = o.kind; P.scalar[k] = o.scalar ? 1 : 0; P.val[k] = o.val; P.bits[k] = o.bits;
        if (o.kind == SNN_MCC_OP_ADD_F32) P.has_add = 1;
    }
    hipLaunchKernelGGL(k_prop_mcc_pipe, dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, P, s, out, B, Nin, N, accumulate);
    return snn_check_launch();
}
