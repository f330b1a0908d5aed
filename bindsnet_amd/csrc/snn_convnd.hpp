// snn_convnd.hpp -- the order-carrying bodies of Conv1dConnection / Conv3dConnection (bindsnet/network/topology.py:540-683,
// :847-1025) and of their PostPre update (bindsnet/learning/learning.py:422-455, :499-559).
//
// Propagation.  F.conv1d / F.conv3d on 0/1 spikes is, per output, ONE sequential f32 chain over the taps in ascending
// (kd, kh, kw) order with the input channel innermost, then + bias (probed on the reference's torch: conv1d at Cin 1..16,
// conv3d at Cin 1).  A silent tap adds w * 0 = +-0, which leaves the chain unchanged, so only the taps whose source spiked are
// visited.  A sample's spikes are packed into one bitstream in channels-last order, bit q = ((d*H + h)*Wd + w)*Cin + ci: for a
// fixed output and (kd, kh) the taps (kw, ci) are then ONE contiguous bit range, whose set bits ascend in exactly the chain's
// order (convnd_chain).  Spike bytes are 0/1, as every layer of this package produces them.
//
// PostPre.  The reference builds the source operand of its bmm by pad + unfold + a raw reshape; that matrix is kept as a
// gather table tab[L, J] (J = Cin*K) of flat source indices, -1 for padding.  Per sample, element (co, j) of the update is
//   pre  = sum_l x_tgt[co, l] * s_src[tab[l, j]]      post = sum_l s_tgt[co, l] * x_src[tab[l, j]]
// summed over l ascending (torch.bmm at these shapes, probed); every product has a 0/1 factor and is exact.  The post term
// walks only the set bits of the target's packed spike words (convnd_pp_post); skipped terms are +0.
//
// The bodies are __host__ __device__: tests/hostcheck/convnd_host.hip runs them on the CPU against torch
// (tests/test_conv_nd_host.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snn {

struct ConvNdGeom { int Cin, D, H, Wd, Cout, KD, KH, KW, stride, pad, padd, padh, OD, OH, OW; };

// The geometry of the C ABI's arguments: an axis of extent 1 with a kernel of 1 is not padded (that is how a conv1d is
// passed: D = H = KD = KH = 1); every other axis takes `pad` on both sides.
__host__ __device__ inline ConvNdGeom convnd_geom(int Cin, int D, int H, int Wd, int Cout, int KD, int KH, int KW, int stride, int pad) {
    const int padd = (D == 1 && KD == 1) ? 0 : pad, padh = (H == 1 && KH == 1) ? 0 : pad;
    return ConvNdGeom{Cin, D, H, Wd, Cout, KD, KH, KW, stride, pad, padd, padh, (D + 2 * padd - KD) / stride + 1,
                      (H + 2 * padh - KH) / stride + 1, (Wd + 2 * pad - KW) / stride + 1};
}

// word k of one sample's channels-last spike bitstream; s is the sample's [Cin, D, H, Wd] spikes, n_src = Cin*D*H*Wd.
// One channel, a whole aligned word: eight independent 4-byte loads (bit i of a nibble = byte i != 0).
__host__ __device__ inline uint32_t convnd_pack_word(const uint8_t *s, const ConvNdGeom &g, long k, long n_src) {
    const long plane = (long)g.D * g.H * g.Wd;
    uint32_t m = 0;
    if (g.Cin == 1 && (k + 1) * 32 <= n_src && ((uintptr_t)(s + k * 32) & 3u) == 0) {
        const uint32_t *p = (const uint32_t *)(s + k * 32);
        uint32_t v[8];
        for (int j = 0; j < 8; ++j) v[j] = p[j];
        for (int j = 0; j < 8; ++j)
            for (int i = 0; i < 4; ++i) m |= (uint32_t)(((v[j] >> (8 * i)) & 0xFFu) != 0) << (4 * j + i);
        return m;
    }
    for (int i = 0; i < 32; ++i) {
        const long q = k * 32 + i;
        if (q >= n_src) break;
        const long pos = g.Cin == 1 ? q : q / g.Cin;
        const int ci = (int)(q - pos * g.Cin);
        m |= (uint32_t)(s[(long)ci * plane + pos] != 0) << i;
    }
    return m;
}

// bits [lo, hi) of word k's range [32k, 32k + 32), hi > 32k
__host__ __device__ inline uint32_t convnd_window(uint32_t m, long k, long lo, long hi) {
    const long b0 = k << 5;
    if (b0 < lo) m &= ~0u << (int)(lo - b0);
    if (hi - b0 < 32) m &= (1u << (int)(hi - b0)) - 1u;
    return m;
}

// The chain of output (od, oh, ow) of one output channel: bits(k) = word k of the sample's bitstream, wgt(i) = element i of
// the channel's [Cin, KD, KH, KW] filter.  Returns the chain before the bias.
template <class BITS, class WGT>
__host__ __device__ inline float convnd_chain(const ConvNdGeom &g, int od, int oh, int ow, BITS bits, WGT wgt) {
    const int HW = g.KH * g.KW, KK = g.KD * HW;
    float acc = 0.f;
    const int w0 = ow * g.stride - g.pad;
    const int wlo = w0 > 0 ? w0 : 0, whi = w0 + g.KW < g.Wd ? w0 + g.KW : g.Wd;
    if (wlo >= whi) return acc;
    for (int kd = 0; kd < g.KD; ++kd) {
        const int d = od * g.stride - g.padd + kd;
        if (d < 0 || d >= g.D) continue;
        for (int kh = 0; kh < g.KH; ++kh) {
            const int h = oh * g.stride - g.padh + kh;
            if (h < 0 || h >= g.H) continue;
            const long row = ((long)d * g.H + h) * g.Wd;                 // position of (d, h, 0)
            const long qlo = (row + wlo) * g.Cin, qhi = (row + whi) * g.Cin, q0 = (row + w0) * g.Cin;
            const int tap0 = kd * HW + kh * g.KW;
            for (long k = qlo >> 5; k <= (qhi - 1) >> 5; ++k) {
                uint32_t m = convnd_window(bits(k), k, qlo, qhi);
                while (m) {
                    const long rel = (k << 5) + __builtin_ctz(m) - q0;   // kw * Cin + ci
                    m &= m - 1;
                    const int kw = g.Cin == 1 ? (int)rel : (int)(rel / g.Cin), ci = (int)(rel - (long)kw * g.Cin);
                    acc = acc + wgt(ci * KK + tap0 + kw);
                }
            }
        }
    }
    return acc;
}

// word k of the packed spikes of one (sample, output channel) row of L target positions
__host__ __device__ inline uint32_t convnd_pack_row_word(const uint8_t *row, int L, int k) {
    uint32_t m = 0;
    for (int i = 0; i < 32 && (k << 5) + i < L; ++i) m |= (uint32_t)(row[(k << 5) + i] != 0) << i;
    return m;
}

// pre term of element j for one (sample, output channel): x_tgt row xt[L], s_at(i) = the sample's source spike i (0/1)
template <class SRC>
__host__ __device__ inline float convnd_pp_pre(const int *tab, int L, int J, int j, const float *xt, SRC s_at) {
    float a = 0.f;
    for (int l = 0; l < L; ++l) {
        const int i = tab[(long)l * J + j];
        const float sv = i >= 0 ? s_at(i) : 0.0f;
        a = a + xt[l] * sv;
    }
    return a;
}

// post term of element j for one (sample, output channel): word(k) = word k of the packed target spikes, x_at(i) = the
// sample's source trace i.  Only the spiking target positions are visited, in ascending l.
template <class WORD, class XSRC>
__host__ __device__ inline float convnd_pp_post(const int *tab, int L, int J, int j, WORD word, XSRC x_at) {
    float p = 0.f;
    for (int k = 0; k < (L + 31) >> 5; ++k) {
        uint32_t m = word(k);
        while (m) {
            const int l = (k << 5) + __builtin_ctz(m);
            m &= m - 1;
            const int i = tab[(long)l * J + j];
            p = p + (i >= 0 ? x_at(i) : 0.0f);                             // 1.0f * x_src
        }
    }
    return p;
}

}  // namespace snn
