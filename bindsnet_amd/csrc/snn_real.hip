// snn_real.hip -- a real-valued (analog) Input layer on the device: its step, and the dense product and the convolution over its
// f32 values (include/snnhip.h, "real-valued Input").  The arithmetic is snn_real.hpp's; nothing here uses the matrix cores or
// splits a chain: every (sample, target) sum stays ONE sequential f32 chain in the stated order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_real.hpp"

using namespace snn;

// =============================================================================================
// Dense.  Workgroup: 256 threads = 4 waves over ONE tile of S target columns (S = 16, 32 or 64: the entry point takes the narrowest
// that keeps the grid within kDenseBlocks workgroups); lane <-> column (lanes beyond S repeat a column and store nothing), wave <->
// its own tile of TB samples, so a workgroup carries 4 * TB samples and one load of W[i, j] serves all of them.  The sources go by
// in chunks of CH = 4096 / S rows: all 256 threads fetch the chunk's [CH, S] block of W (row segments, coalesced; the NEXT chunk's
// loads are in flight while this one is summed) and hand it over through LDS -- with 10 columns the 246 other threads still load --;
// each wave stages its samples' values of the chunk in LDS ([row][TB], read back as broadcasts) and ballots "some sample of my tile
// is non-zero here" per row -- the wave then walks only the set bits, ascending: the wave-uniform skip.
// =============================================================================================
static constexpr int kUnroll = 8;        // rows summed per pass of the walk

template <int TB, int LOGS>
__global__ __launch_bounds__(256) void k_dense_real(const float *__restrict__ W, const float *__restrict__ bias, const float *__restrict__ x,
                                                    float *__restrict__ out, int B, int Nin, int N, int accumulate) {
    constexpr int S = 1 << LOGS, CH = 4096 / S, Q = CH / 64;
    __shared__ float wt[4096];                                         // [CH][S]
    __shared__ __attribute__((aligned(16))) float xs[4][CH][TB];       // [wave][row][sample of the wave's tile]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j0 = (int)blockIdx.x * S, col = lane & (S - 1), j = j0 + col;
    const long b0 = ((long)blockIdx.y * 4 + wave) * TB;
    float acc[TB], wpre[16], xpre[Q][TB];
#pragma unroll
    for (int t = 0; t < TB; ++t) acc[t] = 0.0f;

    auto fetch = [&](int base) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int idx = tid + 256 * k, r = idx >> LOGS, c = idx & (S - 1);
            const int i = base + r, jj = j0 + c;
            wpre[k] = (i < Nin && jj < N) ? W[(size_t)i * N + jj] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int i = base + q * 64 + lane;
#pragma unroll
            for (int t = 0; t < TB; ++t) xpre[q][t] = (i < Nin && b0 + t < B) ? x[(size_t)(b0 + t) * Nin + i] : 0.0f;
        }
    };

    fetch(0);
    for (int base = 0; base < Nin; base += CH) {
        unsigned long long m[Q];
#pragma unroll
        for (int k = 0; k < 16; ++k) wt[tid + 256 * k] = wpre[k];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            bool any = false;
#pragma unroll
            for (int t = 0; t < TB; ++t) { xs[wave][q * 64 + lane][t] = xpre[q][t]; any = any || xpre[q][t] != 0.0f; }
            m[q] = __ballot(any);
        }
        __syncthreads();
        if (base + CH < Nin) fetch(base + CH);
        if (b0 < B) {                                                   // (wave-uniform)
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                unsigned long long mm = m[q];
                while (mm) {                                            // kUnroll rows per pass: their LDS reads are in flight together
                    int r[kUnroll];
                    bool on[kUnroll];
                    float wv[kUnroll], xv[kUnroll][TB];
#pragma unroll
                    for (int u = 0; u < kUnroll; ++u) {
                        on[u] = mm != 0;
                        r[u] = on[u] ? q * 64 + __ffsll((long long)mm) - 1 : q * 64;
                        mm &= mm - 1;                                   // (0 stays 0)
                    }
#pragma unroll
                    for (int u = 0; u < kUnroll; ++u) {
                        wv[u] = wt[(r[u] << LOGS) + col];
#pragma unroll
                        for (int t = 0; t < TB; ++t) xv[u][t] = xs[wave][r[u]][t];
                    }
#pragma unroll
                    for (int u = 0; u < kUnroll; ++u)
                        if (on[u]) {                                    // (wave-uniform: the mask is a ballot)
#pragma unroll
                            for (int t = 0; t < TB; ++t) real_term(acc[t], xv[u][t], wv[u]);
                        }
                }
            }
        }
        __syncthreads();
    }
    if (lane < S && j < N) {
        const float bj = bias ? bias[j] : 0.0f;
#pragma unroll
        for (int t = 0; t < TB; ++t)
            if (b0 + t < B) {
                const size_t o = (size_t)(b0 + t) * N + j;
                out[o] = real_finish(acc[t], bias != nullptr, bj, accumulate, accumulate ? out[o] : 0.0f);
            }
    }
}

static constexpr int kDenseTB = 2;       // samples per wave (measured against 4 and 8: profiles/NOTES_analog.md)
static constexpr long kDenseBlocks = 512;  // (measured against "always 64 columns")

extern "C" int snn_prop_dense_real_f32(const float *W, const float *bias, const float *x, float *out, int B, int Nin, int N,
                                       int accumulate, snn_stream_t stream) {
    if (!W || !x || !out || B <= 0 || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (Nin >= (1 << 24) || B > 65535) return SNN_ERR_UNSUPPORTED;
    const unsigned gy = (unsigned)((B + 4 * kDenseTB - 1) / (4 * kDenseTB));
    // The narrowest column tile that keeps the launch within kDenseBlocks workgroups: a narrow tile spreads few columns over more CUs
    // and takes 4096 / S rows a chunk (fewer exposed load latencies on the chain); a wide one costs fewer wave instructions per sum.
    int logs = 6;
    for (int l = 4; l < 6; ++l)
        if (((long)(N + (1 << l) - 1) >> l) * gy <= kDenseBlocks) { logs = l; break; }
    const dim3 grid((unsigned)((N + (1 << logs) - 1) >> logs), gy);
    hipStream_t st = (hipStream_t)stream;
    if (logs == 4) hipLaunchKernelGGL((k_dense_real<kDenseTB, 4>), grid, dim3(256), 0, st, W, bias, x, out, B, Nin, N, accumulate);
    else if (logs == 5) hipLaunchKernelGGL((k_dense_real<kDenseTB, 5>), grid, dim3(256), 0, st, W, bias, x, out, B, Nin, N, accumulate);
    else hipLaunchKernelGGL((k_dense_real<kDenseTB, 6>), grid, dim3(256), 0, st, W, bias, x, out, B, Nin, N, accumulate);
    return snn_check_launch();
}

// =============================================================================================
// Conv2d, direct.  thread <-> output pixel (b, oy, ox), blockIdx.y <-> a group of 8 output channels, as k_conv2d.  The group's
// filters go to LDS in walking order ([(ky, kx, ci)][8]: one tap's 8 weights are 32 contiguous bytes, read as broadcasts) where
// they fit 32 KiB, the images of the block's samples where they fit 48 KiB; what does not fit is read through L2.
// =============================================================================================
template <bool WLDS>
__global__ __launch_bounds__(256) void k_conv2d_real(const float *__restrict__ W, const float *__restrict__ bias, const float *__restrict__ x,
                                                     float *__restrict__ out, int B, int Cin, int H, int Wd, int Cout, int KH, int KW,
                                                     int stride, int pad, int OH, int OW, int accumulate, int nstage) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int taps = Cin * KH * KW, c0 = (int)blockIdx.y * 8;
    float *wsm = sm, *simg = sm + (WLDS ? (size_t)taps * 8 : 0);
    if (WLDS)
        for (int k = threadIdx.x; k < taps * 8; k += 256) {
            const int o = k >> 3, u = k & 7, ci = o % Cin, kk = o / Cin;           // kk = ky * KW + kx
            wsm[k] = c0 + u < Cout ? W[((size_t)(c0 + u) * Cin + ci) * KH * KW + kk] : 0.0f;
        }
    const long npix = (long)B * OH * OW, p0 = (long)blockIdx.x * 256;
    const int img = Cin * H * Wd, bfirst = (int)(p0 / ((long)OW * OH));
    if (nstage > 0) {
        const long n = (long)min(nstage, B - bfirst) * img;
        const float *src = x + (size_t)bfirst * img;
        for (long k = threadIdx.x; k < n; k += 256) simg[k] = src[k];
    }
    __syncthreads();
    const long p = p0 + threadIdx.x;
    if (p >= npix) return;
    const int ox = (int)(p % OW), oy = (int)((p / OW) % OH), b = (int)(p / ((long)OW * OH));
    const float *sb = nstage > 0 ? simg + (size_t)(b - bfirst) * img : x + (size_t)b * img;
    float acc[8];
    real_conv2d_chains<8>(acc,
        [=](int ci, int iy, int ix) { return sb[((size_t)ci * H + iy) * Wd + ix]; },
        [=](int u, int ci, int ky, int kx) {
            if (WLDS) return wsm[((size_t)(ky * KW + kx) * Cin + ci) * 8 + u];
            return c0 + u < Cout ? W[(((size_t)(c0 + u) * Cin + ci) * KH + ky) * KW + kx] : 0.0f;
        }, Cin, H, Wd, KH, KW, stride, pad, oy, ox);
#pragma unroll
    for (int u = 0; u < 8; ++u)
        if (c0 + u < Cout) {
            const size_t o = (((size_t)b * Cout + c0 + u) * OH + oy) * OW + ox;
            out[o] = real_finish(acc[u], bias != nullptr, bias ? bias[c0 + u] : 0.0f, accumulate, accumulate ? out[o] : 0.0f);
        }
}

extern "C" int snn_prop_conv2d_real_f32(const float *W, const float *bias, const float *x, float *out, int B, int Cin, int H, int Wd,
                                        int Cout, int KH, int KW, int stride, int pad, int accumulate, snn_stream_t stream) {
    if (!W || !x || !out || B <= 0 || Cin <= 0 || H <= 0 || Wd <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0)
        return SNN_ERR_INVALID;
    const long long OHl = ((long long)H + 2ll * pad - KH) / stride + 1, OWl = ((long long)Wd + 2ll * pad - KW) / stride + 1;
    if ((long long)H + 2ll * pad < KH || (long long)Wd + 2ll * pad < KW || OHl <= 0 || OWl <= 0) return SNN_ERR_INVALID;
    if ((long long)Cin * KH * KW > SNN_CONV2D_MAX_TAPS || (long long)Cin * H * Wd > SNN_CONV2D_MAX_IMAGE || OHl * OWl > SNN_CONV2D_MAX_IMAGE)
        return SNN_ERR_UNSUPPORTED;
    const int OH = (int)OHl, OW = (int)OWl;
    const long long blocks = ((long long)B * OH * OW + 255) / 256;
    if (blocks > 0x7fffffffll || (Cout + 7) / 8 > 65535) return SNN_ERR_UNSUPPORTED;
    const long long taps = (long long)Cin * KH * KW, img = (long long)Cin * H * Wd;
    const bool wlds = taps * 8 * 4 <= 32 * 1024;
    long long nstage = 255 / ((long long)OH * OW) + 2;             // a block of 256 consecutive output pixels touches at most that many samples
    if (nstage * img * 4 > 48 * 1024) nstage = 0;
    const size_t lds = (size_t)((wlds ? taps * 8 : 0) + nstage * img) * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {           // up to 32 KiB of filters and 48 KiB of images
        if (snn_check(hipFuncSetAttribute((const void *)k_conv2d_real<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024))) return SNN_ERR_LAUNCH;
        if (snn_check(hipFuncSetAttribute((const void *)k_conv2d_real<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024))) return SNN_ERR_LAUNCH;
        attr_set = true;
    }
    const dim3 grid((unsigned)blocks, (unsigned)((Cout + 7) / 8));
    if (wlds)
        hipLaunchKernelGGL(k_conv2d_real<true>, grid, dim3(256), lds, (hipStream_t)stream, W, bias, x, out, B, Cin, H, Wd, Cout, KH, KW, stride,
                           pad, OH, OW, accumulate, (int)nstage);
    else
        hipLaunchKernelGGL(k_conv2d_real<false>, grid, dim3(256), lds, (hipStream_t)stream, W, bias, x, out, B, Cin, H, Wd, Cout, KH, KW, stride,
                           pad, OH, OW, accumulate, (int)nstage);
    return snn_check_launch();
}

// =============================================================================================
// Input step: the trace of a real-valued Input layer and its f32 raster.  grid (blocks over the N neurons, B samples).
// =============================================================================================
__global__ __launch_bounds__(256) void k_input_real(const float *__restrict__ s, float *__restrict__ x, int N, snn_lif_params p, snn_pervec pv,
                                                    float *__restrict__ raster) {
    const long base = (long)blockIdx.y * N;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < N; j += (long)gridDim.x * 256) {
        const long k = base + j;
        const node_row r = row_of<true>(p, 0.f, pv, j);
        const float sv = s[k];
        if (x) x[k] = real_trace_next(x[k], sv, r.trace_decay, r.trace_scale, p.traces_additive);
        if (raster) raster[k] = sv;
    }
}

extern "C" int snn_input_step_real_pv(const float *s, float *x, int B, int N, float trace_decay, float trace_scale, int additive,
                                      const snn_pervec *pv, float *raster_out, snn_stream_t stream) {
    if (!s || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (pervec_any(pv) && (!x || !pervec_within(pv, kPvTrace) || (pv->v[SNN_PV_TRACE_SCALE] && !additive))) return SNN_ERR_INVALID;
    if (B > 65535) return SNN_ERR_UNSUPPORTED;
    if (!x && !raster_out) return SNN_OK;
    snn_lif_params p = {};
    p.traces = 1; p.trace_decay = trace_decay; p.trace_scale = trace_scale; p.traces_additive = additive;
    snn_pervec none = {};
    const unsigned gx = (unsigned)((N + 255) / 256 < 2048 ? (N + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_input_real, dim3(gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, s, x, N, p, pv ? *pv : none, raster_out);
    return snn_check_launch();
}
