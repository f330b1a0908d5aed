// snn_local.hip -- LocalConnection1D / 2D / 3D (bindsnet/network/topology.py:1488-1910) and their PostPre update
// (bindsnet/learning/learning.py:208-389) on gfx950.
//
// The three classes differ only in the `unfold` calls that gather the source spikes of each receptive field, so both
// kernels take that gather as a table: src[ci, o, k] = flat source index of tap k of receptive field o in input channel
// ci (int32 [Cin, conv_prod, kernel_prod], built on the host by pushing arange(n_src) through the reference's own unfolds).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (csrc/Makefile): every * and + below is one rounding.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_order.hpp"
#include "snn_common.hpp"

using namespace snn;

namespace {

constexpr int kLocalThreads = 256;          // one workgroup = 4 waves; one thread per target neuron (stride loop)
constexpr int kLocalStage = 32 * 1024;      // bytes of LDS for one sample's source spikes; wider sources read global memory
constexpr int kLocalMaxGridX = 1024;

// compute (topology.py:1573-1597 / :1731-1746 / :1880-1896):
//   out[b, r] = sum_ci ( sum_k s[b, src[ci, r % conv_prod, k]] * W[ci, r, k] )
// The inner sum over the kernel_prod taps of one row is ATen's vectorised inner sum (`a_post.sum(-1)`, inner_sum8_terms);
// the sum over input channels (`.sum(1)`) an outer reduction in ascending channel order.  Event-driven: a silent tap
// contributes +0 (the identity on the lane accumulators) and its weight is never loaded.
// grid (min(ceil(R / 256), 1024), B); workgroup <-> sample b, thread <-> target neurons r (stride loop over R = F*conv_prod).
template <bool STAGED>
__global__ __launch_bounds__(kLocalThreads) void k_prop_local(const float *__restrict__ W, const int *__restrict__ src,
                                                              const uint8_t *__restrict__ s, float *__restrict__ out, int Cin,
                                                              int R, int conv_prod, int kernel_prod, int n_src, int accumulate) {
    __shared__ uint8_t staged[STAGED ? kLocalStage : 1];
    const int b = blockIdx.y;
    const uint8_t *srow = s + (size_t)b * n_src;
    if (STAGED) {
        for (int i = threadIdx.x; i < n_src; i += kLocalThreads) staged[i] = srow[i];
        __syncthreads();
    }
    const uint8_t *spk = STAGED ? staged : srow;
    for (int r = blockIdx.x * kLocalThreads + threadIdx.x; r < R; r += gridDim.x * kLocalThreads) {
        const int o = r % conv_prod;
        float acc = 0.f;
        for (int ci = 0; ci < Cin; ++ci) {
            const int *tab = src + ((size_t)ci * conv_prod + o) * kernel_prod;
            const float *w = W + ((size_t)ci * R + r) * kernel_prod;
            const float row = inner_sum8_terms([&](int k) {
                const int i = tab[k];
                return ((unsigned)i < (unsigned)n_src && spk[i]) ? w[k] : 0.0f;
            }, kernel_prod);
            acc = acc + row;
        }
        float *dst = out + (size_t)b * R + r;
        *dst = accumulate ? *dst + acc : 0.0f + acc;
    }
}

// PostPre (learning.py:208-389 + LearningRule.update :87-104).  W is the flat [R = F*conv_prod, J = Cin*kernel_prod]
// matrix the reference's `pre.view(w.size())` writes into: element (r, j) takes the source at flat unfolded position
// p = (r % conv_prod) * J + j of the [Cin, conv_prod, kernel_prod] unfold, decoded as (ci, o, k) and looked up in src.
// Each bmm element has exactly one non-zero product, so pre[b, r, j] = x_tgt[b, r] * s_src[b, src(r, j)] and
// post[b, r, j] = s_tgt[b, r] * x_src[b, src(r, j)] exactly; the batch reduction is ATen's sum(dim=0) order over the
// W.numel() columns (batch_sum; one term at B = 1 == torch.squeeze).  Then w - nu0*pre, w + nu1*post (each half only when its
// rate is non-zero), w * decay, clamp.  One thread per weight element (grid-stride); every weight is read and written once.
// RED: the batch reduction (snn_order.hpp batch_sum<R>; SUM is the function as it was).
template <int RED = kReduceSum>
__global__ __launch_bounds__(kLocalThreads) void k_local_postpre(float *__restrict__ W, const int *__restrict__ src,
                                                                 const uint8_t *__restrict__ s_src, const float *__restrict__ x_src,
                                                                 const uint8_t *__restrict__ s_tgt, const float *__restrict__ x_tgt,
                                                                 int B, int Cin, int R, int conv_prod, int kernel_prod, int n_src,
                                                                 float nu0, float nu1, float decay, int has_min, float wmin,
                                                                 int has_max, float wmax) {
    const long J = (long)Cin * kernel_prod, E = (long)R * J, CK = (long)conv_prod * kernel_prod;
    for (long e = (long)blockIdx.x * kLocalThreads + threadIdx.x; e < E; e += (long)gridDim.x * kLocalThreads) {
        const int r = (int)(e / J);
        const long j = e - (long)r * J;
        const long p = (long)(r % conv_prod) * J + j;
        const int ci = (int)(p / CK);
        const long rem = p - (long)ci * CK;
        const int o = (int)(rem / kernel_prod), k = (int)(rem - (long)o * kernel_prod);
        const int si = src[((size_t)ci * conv_prod + o) * kernel_prod + k];
        const bool in = (unsigned)si < (unsigned)n_src;
        const int sc = in ? si : 0;
        float w = W[e];
        if (nu0 != 0.f) {
            const float pre = batch_sum<RED>([&](int b) {
                const float sv = in ? (float)s_src[(size_t)b * n_src + sc] : 0.0f;
                return x_tgt[(size_t)b * R + r] * sv;
            }, B, e, E);
            const float u = nu0 * pre;
            w = w - u;
        }
        if (nu1 != 0.f) {
            const float post = batch_sum<RED>([&](int b) {
                const float xv = in ? x_src[(size_t)b * n_src + sc] : 0.0f;
                return (float)s_tgt[(size_t)b * R + r] * xv;
            }, B, e, E);
            const float u = nu1 * post;
            w = w + u;
        }
        w = w * decay;
        if (has_min && w < wmin) w = wmin;
        if (has_max && w > wmax) w = wmax;
        W[e] = w;
    }
}

}  // namespace

extern "C" int snn_prop_local_f32(const float *W, const int *src, const uint8_t *s, float *out, int B, int Cin, int F,
                                  int conv_prod, int kernel_prod, int n_src, int accumulate, snn_stream_t stream) {
    if (!W || !src || !s || !out || B <= 0 || Cin <= 0 || F <= 0 || conv_prod <= 0 || kernel_prod <= 0 || n_src <= 0)
        return SNN_ERR_INVALID;
    const long R = (long)F * conv_prod;
    if (R > (1L << 30) || (long)Cin * R * kernel_prod > (1L << 40) || B > 65535) return SNN_ERR_UNSUPPORTED;
    const long gx = (R + kLocalThreads - 1) / kLocalThreads;
    const dim3 grid((unsigned)(gx < kLocalMaxGridX ? gx : kLocalMaxGridX), (unsigned)B);
    if (n_src <= kLocalStage)
        hipLaunchKernelGGL(k_prop_local<true>, grid, dim3(kLocalThreads), 0, (hipStream_t)stream, W, src, s, out, Cin, (int)R, conv_prod,
                           kernel_prod, n_src, accumulate);
    else
        hipLaunchKernelGGL(k_prop_local<false>, grid, dim3(kLocalThreads), 0, (hipStream_t)stream, W, src, s, out, Cin, (int)R, conv_prod,
                           kernel_prod, n_src, accumulate);
    return snn_check_launch();
}

extern "C" int snn_local_postpre_red(float *W, const int *src, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                                     const float *x_tgt, int B, int Cin, int F, int conv_prod, int kernel_prod, int n_src, float nu0,
                                     float nu1, float decay, int has_min, float wmin, int has_max, float wmax, int reduce,
                                     snn_stream_t stream) {
    if (reduce < SNN_REDUCE_SUM || reduce > SNN_REDUCE_AMIN) return SNN_ERR_INVALID;
    if (!W || !src || !s_src || !x_src || !s_tgt || !x_tgt || B <= 0 || Cin <= 0 || F <= 0 || conv_prod <= 0 || kernel_prod <= 0 ||
        n_src <= 0)
        return SNN_ERR_INVALID;
    const long R = (long)F * conv_prod, E = (long)Cin * R * kernel_prod;
    if (R > (1L << 30) || E > (1L << 40) || B > kMaxTerms) return SNN_ERR_UNSUPPORTED;
    const long g = (E + kLocalThreads - 1) / kLocalThreads;
    const unsigned grid = (unsigned)(g < 4096 ? g : 4096);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kLocalThreads), 0, (hipStream_t)stream, W, src, s_src, x_src, s_tgt, x_tgt, B,
                           Cin, (int)R, conv_prod, kernel_prod, n_src, nu0, nu1, decay, has_min, wmin, has_max, wmax);
    };
    if (reduce == SNN_REDUCE_MEAN) launch(k_local_postpre<kReduceMean>);
    else if (reduce == SNN_REDUCE_AMAX) launch(k_local_postpre<kReduceAmax>);
    else if (reduce == SNN_REDUCE_AMIN) launch(k_local_postpre<kReduceAmin>);
    else launch(k_local_postpre<>);
    return snn_check_launch();
}

extern "C" int snn_local_postpre(float *W, const int *src, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                                 const float *x_tgt, int B, int Cin, int F, int conv_prod, int kernel_prod, int n_src, float nu0,
                                 float nu1, float decay, int has_min, float wmin, int has_max, float wmax, snn_stream_t stream) {
    return snn_local_postpre_red(W, src, s_src, x_src, s_tgt, x_tgt, B, Cin, F, conv_prod, kernel_prod, n_src, nu0, nu1, decay, has_min, wmin,
                                 has_max, wmax, SNN_REDUCE_SUM, stream);
}
