// snn_average.hip -- the time-averaged (average_update = K) forms of PostPre, MSTDP and MSTDPET on a MulticompartmentConnection's
// Weight (MCC_learning.py:211-289, :457-535, :641-713); the per-element bodies are in snn_average.hpp.
//
// Tiling: a flat grid-stride pass, one thread per weight element, consecutive threads on consecutive elements.  The step's traffic is
// the rings: every step writes one [Nin, N] slot per term, a due step reads all K of them (K * E floats per term, 12.5 MB at 784 x 400,
// K = 10) and nothing of that is shared between elements, so there is nothing for a tile to stage; each slot is a contiguous row-major
// stream and a wave reads 256 consecutive bytes of it.  The batch-side factors (B * (Nin + N) values) are small enough to stay in L2:
// a wave reads one source value (the same address for all its lanes but at a row change) and 64 consecutive target values per sample.
// The 16 x TJ tile of k_plasticity pays off where the batch factors are the traffic; here they are not.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_average.hpp"

using namespace snn;

namespace {

constexpr unsigned kAvgMaxGrid = 4096;

unsigned avg_grid(long n) {
    const long g = (n + 255) / 256;
    return (unsigned)(g < (long)kAvgMaxGrid ? (g > 0 ? g : 1) : (long)kAvgMaxGrid);
}

template <int R = kReduceSum>
__global__ __launch_bounds__(256) void k_avg_postpre(float *W, const AvgPostPre a) {
    const long E = (long)a.Nin * a.N;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long)gridDim.x * 256) avg_postpre_elem<R>(W, a, e);
}

template <int R = kReduceSum>
__global__ __launch_bounds__(256) void k_avg_mstdp(float *W, const AvgMstdp a) {
    const long E = (long)a.Nin * a.N;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long)gridDim.x * 256) avg_mstdp_elem<R>(W, a, e);
}

__global__ __launch_bounds__(256) void k_avg_mstdpet(float *W, const AvgMstdpet a) {
    const long E = (long)a.Nin * a.N;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long)gridDim.x * 256) avg_mstdpet_elem(W, a, e);
}

// The factors of the next eligibility.  A launch of its own behind the weight pass: every weight element reads the OLD factors of its
// row and column, and nothing orders the workgroups of one launch.
__global__ __launch_bounds__(256) void k_avg_traces(float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                                                    const uint8_t *s_tgt, long n_src, long n_tgt, float a_plus, float a_minus, float d_plus,
                                                    float d_minus) {
    const long n = n_src + n_tgt;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256)
        avg_trace_elem(p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, n_src, k, a_plus, a_minus, d_plus, d_minus);
}

bool ring_ok(const float *ring, int K, int continuous, int idx) {
    return ring && K >= 1 && idx >= 0 && idx < K && (continuous == 0 || continuous == 1);
}

}  // namespace

extern "C" int snn_postpre_avg_step_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                                        int Nin, int N, float nu0, float nu1, float dt, float decay, int has_min, float wmin, int has_max,
                                        float wmax, int squeeze, float *ring_pre, float *ring_post, int K, int continuous, int idx_pre,
                                        int idx_post, int reduce, snn_stream_t stream) {
    if (reduce < SNN_REDUCE_SUM || reduce > SNN_REDUCE_AMIN) return SNN_ERR_INVALID;
    if (!W || !s_src || !x_src || !s_tgt || !x_tgt || B <= 0 || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (!ring_ok(ring_pre, K, continuous, idx_pre) || !ring_ok(ring_post, K, continuous, idx_post)) return SNN_ERR_INVALID;
    if (squeeze && B != 1) return SNN_ERR_INVALID;
    if (K > kAvgMaxTerms || B > kAvgMaxTerms) return SNN_ERR_UNSUPPORTED;
    AvgPostPre a;
    a.s_src = s_src; a.x_src = x_src; a.s_tgt = s_tgt; a.x_tgt = x_tgt;
    a.B = B; a.Nin = Nin; a.N = N;
    a.nu0 = nu0; a.nu1 = nu1; a.dt = dt; a.squeeze = squeeze ? 1 : 0;
    a.fin = AvgBounds{decay, has_min, wmin, has_max, wmax};
    a.pre = avg_ring(ring_pre, K, idx_pre, continuous);
    a.post = avg_ring(ring_post, K, idx_post, continuous);
    auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(avg_grid((long)Nin * N)), dim3(256), 0, (hipStream_t)stream, W, a); };
    if (reduce == SNN_REDUCE_MEAN) launch(k_avg_postpre<kReduceMean>);
    else if (reduce == SNN_REDUCE_AMAX) launch(k_avg_postpre<kReduceAmax>);
    else if (reduce == SNN_REDUCE_AMIN) launch(k_avg_postpre<kReduceAmin>);
    else launch(k_avg_postpre<>);
    return snn_check_launch();
}

extern "C" int snn_postpre_avg_step(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                                    int Nin, int N, float nu0, float nu1, float dt, float decay, int has_min, float wmin, int has_max,
                                    float wmax, int squeeze, float *ring_pre, float *ring_post, int K, int continuous, int idx_pre,
                                    int idx_post, snn_stream_t stream) {
    return snn_postpre_avg_step_red(W, s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, dt, decay, has_min, wmin, has_max, wmax, squeeze,
                                    ring_pre, ring_post, K, continuous, idx_pre, idx_post, SNN_REDUCE_SUM, stream);
}

extern "C" int snn_mstdp_avg_step_red(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                                      const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0,
                                      float a_plus, float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin,
                                      int has_max, float wmax, int squeeze, float *ring, int K, int continuous, int idx, int reduce,
                                      snn_stream_t stream) {
    if (reduce < SNN_REDUCE_SUM || reduce > SNN_REDUCE_AMIN) return SNN_ERR_INVALID;
    if (!W || !p_plus || !p_minus || !s_src_prev || !s_tgt_prev || !s_src || !s_tgt || B <= 0 || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (!ring_ok(ring, K, continuous, idx) || (squeeze && B != 1)) return SNN_ERR_INVALID;
    if (K > kAvgMaxTerms || B > kAvgMaxTerms) return SNN_ERR_UNSUPPORTED;
    AvgMstdp a;
    a.p_plus = p_plus; a.p_minus = p_minus; a.s_src_prev = s_src_prev; a.s_tgt_prev = s_tgt_prev;
    a.B = B; a.Nin = Nin; a.N = N;
    a.reward = reward; a.reward_vec = reward_vec; a.nu0 = nu0; a.squeeze = squeeze ? 1 : 0;
    a.fin = AvgBounds{wdecay, has_min, wmin, has_max, wmax};
    a.ring = avg_ring(ring, K, idx, continuous);
    auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(avg_grid((long)Nin * N)), dim3(256), 0, (hipStream_t)stream, W, a); };
    if (reduce == SNN_REDUCE_MEAN) launch(k_avg_mstdp<kReduceMean>);
    else if (reduce == SNN_REDUCE_AMAX) launch(k_avg_mstdp<kReduceAmax>);
    else if (reduce == SNN_REDUCE_AMIN) launch(k_avg_mstdp<kReduceAmin>);
    else launch(k_avg_mstdp<>);
    int rc = snn_check_launch();
    if (rc) return rc;
    const long n = (long)B * ((long)Nin + N);
    hipLaunchKernelGGL(k_avg_traces, dim3(avg_grid(n)), dim3(256), 0, (hipStream_t)stream, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src,
                       s_tgt, (long)B * Nin, (long)B * N, a_plus, a_minus, decay_plus, decay_minus);
    return snn_check_launch();
}

extern "C" int snn_mstdp_avg_step(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                                  const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0,
                                  float a_plus, float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin,
                                  int has_max, float wmax, int squeeze, float *ring, int K, int continuous, int idx,
                                  snn_stream_t stream) {
    return snn_mstdp_avg_step_red(W, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, B, Nin, N, reward, reward_vec, nu0, a_plus, a_minus,
                                  decay_plus, decay_minus, wdecay, has_min, wmin, has_max, wmax, squeeze, ring, K, continuous, idx,
                                  SNN_REDUCE_SUM, stream);
}

extern "C" int snn_mstdpet_avg_step(float *W, float *e_trace, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev,
                                    const uint8_t *s_src, const uint8_t *s_tgt, int Nin, int N, float reward, float nu0, float dt,
                                    float a_plus, float a_minus, float decay_plus, float decay_minus, float decay_e, float tc_e,
                                    float wdecay, int has_min, float wmin, int has_max, float wmax, float *ring, int K, int continuous,
                                    int idx, snn_stream_t stream) {
    if (!W || !e_trace || !p_plus || !p_minus || !s_src_prev || !s_tgt_prev || !s_src || !s_tgt || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (!ring_ok(ring, K, continuous, idx)) return SNN_ERR_INVALID;
    if (K > kAvgMaxTerms) return SNN_ERR_UNSUPPORTED;
    AvgMstdpet a;
    a.e_trace = e_trace; a.p_plus = p_plus; a.p_minus = p_minus; a.s_src_prev = s_src_prev; a.s_tgt_prev = s_tgt_prev;
    a.Nin = Nin; a.N = N;
    a.scale = (nu0 * dt) * reward;                      // ((nu[0] * dt) * reward) * eligibility_trace, as snn_mstdpet_step
    a.decay_e = decay_e; a.tc_e = tc_e;
    a.fin = AvgBounds{wdecay, has_min, wmin, has_max, wmax};
    a.ring = avg_ring(ring, K, idx, continuous);
    hipLaunchKernelGGL(k_avg_mstdpet, dim3(avg_grid((long)Nin * N)), dim3(256), 0, (hipStream_t)stream, W, a);
    int rc = snn_check_launch();
    if (rc) return rc;
    const long n = (long)Nin + N;
    hipLaunchKernelGGL(k_avg_traces, dim3(avg_grid(n)), dim3(256), 0, (hipStream_t)stream, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src,
                       s_tgt, (long)Nin, (long)N, a_plus, a_minus, decay_plus, decay_minus);
    return snn_check_launch();
}
