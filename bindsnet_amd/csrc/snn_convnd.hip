// snn_convnd.hip -- Conv1dConnection / Conv3dConnection (bindsnet/network/topology.py:540-683, :847-1025) and their PostPre
// update (bindsnet/learning/learning.py:422-455, :499-559) on gfx950.  A conv1d is the conv3d with D = H = KD = KH = 1.
// The summation orders and the event-driven walks are the bodies of snn_convnd.hpp.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (csrc/Makefile): every * and + below is one rounding.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_order.hpp"
#include "snn_common.hpp"
#include "snn_convnd.hpp"

using namespace snn;

namespace {

constexpr int kThreads = 256;
constexpr int kWStage = 12 * 1024;          // floats of LDS for the filters of a workgroup's output channels (48 KiB)
constexpr int kSStage = 4 * 1024;           // words of LDS for one sample's spike bitstream (16 KiB: n_src <= 131 072)
constexpr int kMaskStage = 8 * 1024;        // words of LDS for the packed target spikes of every (sample, channel) (32 KiB)

// compute: thread <-> one output (b, co, p) of a tile of nco output channels x PB positions (nco * PB <= 256); grid (channel
// chunks * position blocks, B).  STAGE_W: the tile's filters in LDS (Cin*K <= kWStage), else read from L2.  STAGE_S: the
// sample's bitstream packed into LDS by the workgroup, else every word is packed where it is read, from global memory.
template <bool STAGE_W, bool STAGE_S>
__global__ __launch_bounds__(kThreads) void k_prop_convnd(const float *__restrict__ W, const float *__restrict__ bias,
                                                          const uint8_t *__restrict__ s, float *__restrict__ out, ConvNdGeom g,
                                                          int PB, int nco, int accumulate) {
    __shared__ float wsm[STAGE_W ? kWStage : 1];
    __shared__ uint32_t bsm[STAGE_S ? kSStage : 1];
    const int P = g.OD * g.OH * g.OW, taps = g.Cin * g.KD * g.KH * g.KW;
    const int npb = (P + PB - 1) / PB, chunk = blockIdx.x / npb, pblk = blockIdx.x - chunk * npb;
    const int co0 = chunk * nco, nc = min(nco, g.Cout - co0), b = blockIdx.y;
    const long n_src = (long)g.Cin * g.D * g.H * g.Wd;
    const uint8_t *sb = s + (size_t)b * n_src;
    if (STAGE_W)                                     // eight loads in flight per thread, then their stores
        for (int k0 = threadIdx.x; k0 < nc * taps; k0 += 8 * kThreads) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = k0 + u * kThreads < nc * taps ? W[(size_t)co0 * taps + k0 + u * kThreads] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) if (k0 + u * kThreads < nc * taps) wsm[k0 + u * kThreads] = v[u];
        }
    if (STAGE_S)
        for (long k = threadIdx.x; k < (n_src + 31) >> 5; k += kThreads) bsm[k] = convnd_pack_word(sb, g, k, n_src);
    if (STAGE_W || STAGE_S) __syncthreads();
    const int cl = threadIdx.x / PB, p = pblk * PB + (threadIdx.x - cl * PB);
    if (cl >= nc || p >= P) return;
    const int co = co0 + cl;
    const int ow = p % g.OW, oh = (p / g.OW) % g.OH, od = p / (g.OW * g.OH);
    const float *wf = STAGE_W ? wsm + cl * taps : W + (size_t)co * taps;
    const float acc = convnd_chain(g, od, oh, ow,
                                   [&](long k) { return STAGE_S ? bsm[k] : convnd_pack_word(sb, g, k, n_src); },
                                   [&](int i) { return wf[i]; });
    const float r = bias ? acc + bias[co] : acc;
    float *dst = out + ((size_t)b * g.Cout + co) * P + p;
    *dst = (accumulate ? *dst : 0.0f) + r;
}

// the packed target spikes of every (sample, output channel) row, [B*Cout, nw] words: the global-memory form of the masks
__global__ __launch_bounds__(kThreads) void k_convnd_pack_tgt(const uint8_t *__restrict__ s_tgt, uint32_t *__restrict__ masks, long rows,
                                                              int L) {
    const int nw = (L + 31) >> 5;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < rows * nw; k += (long)gridDim.x * kThreads) {
        const long r = k / nw;
        masks[k] = convnd_pack_row_word(s_tgt + (size_t)r * L, L, (int)(k - r * nw));
    }
}

// PostPre: one thread per weight element e = co*J + j (grid-stride), every weight read and written once.  Per sample the
// pre / post terms of snn_convnd.hpp, then the batch reduction in ATen's sum(dim=0) order (batch_sum; one term at B = 1,
// where the reference squeezes), then w - nu0*pre (nu0 != 0), w + nu1*post (nu1 != 0), w * decay, clamp
// (learning.py:87-104).  STAGED: the workgroup packs the target masks into LDS itself; else they come from k_convnd_pack_tgt.
// R: the batch reduction (snn_order.hpp batch_sum<R>; SUM is the function as it was).
template <bool STAGED, int R = kReduceSum>
__global__ __launch_bounds__(kThreads) void k_convnd_postpre(float *__restrict__ W, const int *__restrict__ tab,
                                                             const uint8_t *__restrict__ s_src, const float *__restrict__ x_src,
                                                             const uint8_t *__restrict__ s_tgt, const float *__restrict__ x_tgt,
                                                             const uint32_t *__restrict__ gmask, int B, int Cout, int L, int J,
                                                             int n_src, float nu0, float nu1, float decay, int has_min, float wmin,
                                                             int has_max, float wmax) {
    __shared__ uint32_t smask[STAGED ? kMaskStage : 1];
    const int nw = (L + 31) >> 5;
    if (STAGED && nu1 != 0.f) {
        for (int k = threadIdx.x; k < B * Cout * nw; k += kThreads) {
            const int r = k / nw;
            smask[k] = convnd_pack_row_word(s_tgt + (size_t)r * L, L, k - r * nw);
        }
        __syncthreads();
    }
    const uint32_t *masks = STAGED ? smask : gmask;
    const long E = (long)Cout * J;
    for (long e = (long)blockIdx.x * kThreads + threadIdx.x; e < E; e += (long)gridDim.x * kThreads) {
        const int co = (int)(e / J), j = (int)(e - (long)co * J);
        float w = W[e];
        if (nu0 != 0.f) {
            const float pre = batch_sum<R>([&](int b) {
                const uint8_t *ss = s_src + (size_t)b * n_src;
                return convnd_pp_pre(tab, L, J, j, x_tgt + ((size_t)b * Cout + co) * L, [&](int i) { return (float)ss[i]; });
            }, B, e, E);
            const float u = nu0 * pre;
            w = w - u;
        }
        if (nu1 != 0.f) {
            const float post = batch_sum<R>([&](int b) {
                const uint32_t *mk = masks + ((size_t)b * Cout + co) * nw;
                const float *xs = x_src + (size_t)b * n_src;
                return convnd_pp_post(tab, L, J, j, [&](int k) { return mk[k]; }, [&](int i) { return xs[i]; });
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

extern "C" int snn_prop_convnd_f32(const float *W, const float *bias, const uint8_t *s, float *out, int B, int Cin, int D, int H, int Wd,
                                   int Cout, int KD, int KH, int KW, int stride, int pad, int accumulate, snn_stream_t stream) {
    if (!W || !s || !out || B <= 0 || Cin <= 0 || D <= 0 || H <= 0 || Wd <= 0 || Cout <= 0 || KD <= 0 || KH <= 0 || KW <= 0 ||
        stride <= 0 || pad < 0)
        return SNN_ERR_INVALID;
    const ConvNdGeom g = convnd_geom(Cin, D, H, Wd, Cout, KD, KH, KW, stride, pad);
    if (D + 2 * g.padd < KD || H + 2 * g.padh < KH || Wd + 2 * pad < KW) return SNN_ERR_INVALID;
    if (Cin > 16) return SNN_ERR_UNSUPPORTED;     // the reference's accumulation order is only characterised up to 16 channels
    const long n_src = (long)Cin * D * H * Wd, P = (long)g.OD * g.OH * g.OW, taps = (long)Cin * KD * KH * KW;
    if (n_src > (1L << 30) || P > (1L << 30) || taps > (1L << 30) || B > 65535) return SNN_ERR_UNSUPPORTED;
    const int PB = (int)(P < kThreads ? P : kThreads);
    const bool stage_w = taps <= kWStage, stage_s = (n_src + 31) / 32 <= kSStage;
    int nco = kThreads / PB;
    if (nco > Cout) nco = Cout;
    if (stage_w && nco > kWStage / taps) nco = (int)(kWStage / taps);
    const long tiles = (long)((Cout + nco - 1) / nco) * ((P + PB - 1) / PB);
    if (tiles > (1L << 31) - 1) return SNN_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)tiles, (unsigned)B);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, (hipStream_t)stream, W, bias, s, out, g, PB, nco, accumulate);
    };
    if (stage_w && stage_s) launch(k_prop_convnd<true, true>);
    else if (stage_w) launch(k_prop_convnd<true, false>);
    else if (stage_s) launch(k_prop_convnd<false, true>);
    else launch(k_prop_convnd<false, false>);
    return snn_check_launch();
}

// One launch of k_convnd_postpre<STAGED, R> for each of the four reductions.
template <bool STAGED>
static void launch_convnd_postpre(int reduce, dim3 grid, hipStream_t st, float *W, const int *pp_src, const uint8_t *s_src, const float *x_src,
                                  const uint8_t *s_tgt, const float *x_tgt, const uint32_t *masks, int B, int Cout, int L, int J, int n_src,
                                  float nu0, float nu1, float decay, int has_min, float wmin, int has_max, float wmax) {
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, st, W, pp_src, s_src, x_src, s_tgt, x_tgt, masks, B, Cout, L, J, n_src, nu0, nu1,
                           decay, has_min, wmin, has_max, wmax);
    };
    if (reduce == SNN_REDUCE_MEAN) launch(k_convnd_postpre<STAGED, kReduceMean>);
    else if (reduce == SNN_REDUCE_AMAX) launch(k_convnd_postpre<STAGED, kReduceAmax>);
    else if (reduce == SNN_REDUCE_AMIN) launch(k_convnd_postpre<STAGED, kReduceAmin>);
    else launch(k_convnd_postpre<STAGED>);
}

extern "C" int snn_convnd_postpre_red(float *W, const int *pp_src, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                                      const float *x_tgt, int B, int Cout, int L, int J, int n_src, float nu0, float nu1, float decay,
                                      int has_min, float wmin, int has_max, float wmax, uint32_t *ws, int reduce, snn_stream_t stream) {
    if (reduce < SNN_REDUCE_SUM || reduce > SNN_REDUCE_AMIN) return SNN_ERR_INVALID;
    if (!W || !pp_src || !s_src || !x_src || !s_tgt || !x_tgt || B <= 0 || Cout <= 0 || L <= 0 || J <= 0 || n_src <= 0)
        return SNN_ERR_INVALID;
    const long E = (long)Cout * J, nw = (L + 31) / 32, words = (long)B * Cout * nw;
    if (E > (1L << 40) || (long)L * J > (1L << 31) - 1 || B > kMaxTerms) return SNN_ERR_UNSUPPORTED;
    const bool staged = words <= kMaskStage;
    if (!staged && nu1 != 0.f && !ws) return SNN_ERR_INVALID;
    const long g = (E + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(g < 4096 ? g : 4096));
    if (staged) {
        launch_convnd_postpre<true>(reduce, grid, (hipStream_t)stream, W, pp_src, s_src, x_src, s_tgt, x_tgt, (const uint32_t *)nullptr, B, Cout,
                                    L, J, n_src, nu0, nu1, decay, has_min, wmin, has_max, wmax);
    } else {
        if (nu1 != 0.f) {
            const long pg = (words + kThreads - 1) / kThreads;
            hipLaunchKernelGGL(k_convnd_pack_tgt, dim3((unsigned)(pg < 4096 ? pg : 4096)), dim3(kThreads), 0, (hipStream_t)stream, s_tgt, ws,
                               (long)B * Cout, L);
        }
        launch_convnd_postpre<false>(reduce, grid, (hipStream_t)stream, W, pp_src, s_src, x_src, s_tgt, x_tgt, (const uint32_t *)ws, B, Cout, L,
                                     J, n_src, nu0, nu1, decay, has_min, wmin, has_max, wmax);
    }
    return snn_check_launch();
}

extern "C" int snn_convnd_postpre(float *W, const int *pp_src, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                                  const float *x_tgt, int B, int Cout, int L, int J, int n_src, float nu0, float nu1, float decay,
                                  int has_min, float wmin, int has_max, float wmax, uint32_t *ws, snn_stream_t stream) {
    return snn_convnd_postpre_red(W, pp_src, s_src, x_src, s_tgt, x_tgt, B, Cout, L, J, n_src, nu0, nu1, decay, has_min, wmin, has_max, wmax, ws,
                                  SNN_REDUCE_SUM, stream);
}
