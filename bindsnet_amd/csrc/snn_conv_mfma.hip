// snn_conv_mfma.hip -- Conv2dConnection.compute over spike bytes as an implicit GEMM on v_mfma_f32_16x16x4_f32: the order, the reason
// the bits are those of snn_prop_conv2d_f32, the LDS layouts and the bank argument are in snn_conv_mfma.hpp, whose bodies this kernel
// calls.
//
// grid.x = (blocks of 64 consecutive output pixels of the flattened [B, OH, OW]) x (groups of 16 NT output channels), the groups of a
// block adjacent so that they read the same input bands out of L2; 256 threads = 4 waves.  Wave w owns the block's pixel tile w and the
// NT channel tiles of the group: NT accumulators (f32x4) that live in registers from tap 0 to the last tap -- no split-K, nothing merged
// in --, fed by ONE A fragment per MFMA step, so that NT independent chains hide each other's MFMA latency.
// K is walked tap by tap, 16 (padded) channels = one round of four MFMAs at a time, in slabs of 4 rounds: while slab i feeds the
// chains out of one LDS buffer, slab i + 1's weights are in flight from global memory into registers and are written, transposed to
// [term][channel], into the other buffer behind the round; one barrier per slab.  No repack kernel, no packed copy: the weights may change
// between calls.
// The workgroup's census of the bytes it staged decides its body in the same launch: all 0/1 -> the chains; else scalar_output per thread.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_conv_mfma.hpp"

using namespace snn;
namespace cm = snn::conv_mfma;
namespace da = snn::dense_auto;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int NT>
__global__ __launch_bounds__(cm::kWaves * 64) void k_conv_mfma(const float *__restrict__ W, const float *__restrict__ bias,
                                                               const uint8_t *__restrict__ s, float *__restrict__ out, int B, WideGeom g,
                                                               int accumulate, int *__restrict__ counters, int ngroups) {
    constexpr int RS = cm::slab_stride(NT), SF = cm::slab_floats(NT), NTHREADS = cm::kWaves * 64, PER = cm::kSlabRows * 16 * NT / NTHREADS;
    extern __shared__ __align__(16) unsigned char cm_lds[];
    float *slab = (float *)cm_lds;                                                  // [2][kSlabRows][RS]
    uint8_t *bands = cm_lds + 2 * SF * sizeof(float);                               // [samples of the block][band_bytes]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = (int)(blockIdx.x % (unsigned)ngroups) * 16 * NT;
    const long p0 = (long)(blockIdx.x / (unsigned)ngroups) * cm::kBlockPix;
    const int nps = g.OH * g.OW, hw = g.H * g.Wd, CPB = cm::padded_channels(g.Cin) / 16;
    const long npix = (long)B * nps;
    const size_t img = (size_t)g.Cin * hw;
    const int rounds = g.KH * g.KW * CPB, nslab = (rounds + 3) / 4;
    const long plast = p0 + cm::kBlockPix - 1 < npix - 1 ? p0 + cm::kBlockPix - 1 : npix - 1;
    const int bfirst = (int)(p0 / nps), nsm = (int)(plast / nps) - bfirst + 1;
    const size_t slot_bytes = (size_t)cm::band_bytes(g);

    // the bands of the block's samples, and their census
    da::census cen = {0, 0};
    for (int sm = 0; sm < nsm; ++sm)
        cm::stage_band((uint32_t *)(bands + sm * slot_bytes), s + (size_t)(bfirst + sm) * img, g, cm::band_of(p0, npix, bfirst + sm, g), tid,
                       NTHREADS, cen);
    // slab `sl` of the group's weights: into registers (loads of valid addresses only), then transposed into buffer sl & 1
    float wr[PER];
    auto load_slab = [&](int sl) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const cm::SlabSlot e = cm::slab_slot(tid + i * NTHREADS);
            wr[i] = cm::slab_weight(W, g, (long long)sl * cm::kSlabRows + e.row, c0 + e.col);
        }
    };
    auto store_slab = [&](int sl) __attribute__((always_inline)) {
        float *dst = slab + (sl & 1) * SF;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const cm::SlabSlot e = cm::slab_slot(tid + i * NTHREADS);
            dst[e.row * RS + e.col] = wr[i];
        }
    };
    load_slab(0);
    store_slab(0);
    const int scalar = __syncthreads_or(cen.above1);                                // (the bands and slab 0 are visible behind it)
    if (tid == 0 && counters) atomicAdd(&counters[scalar ? 1 : 0], 1);

    if (scalar) {                                                                   // (uniform) a byte above 1: the stated order, thread by thread
        for (int o = tid; o < cm::kBlockPix * 16 * NT; o += NTHREADS) {
            const long p = p0 + (o & (cm::kBlockPix - 1));                          // consecutive threads: consecutive pixels of one channel
            const int co = c0 + o / cm::kBlockPix;
            if (p >= npix || co >= g.Cout) continue;
            const int b = (int)(p / nps), pin = (int)(p - (long)b * nps), oy = pin / g.OW, ox = pin - oy * g.OW;
            const float acc = cm::scalar_output(bands + (b - bfirst) * slot_bytes, cm::band_of(p0, npix, b, g), g, oy, ox, W, co);
            const size_t at = ((size_t)b * g.Cout + co) * nps + pin;
            out[at] = wide_emit(acc, bias, co, accumulate ? out[at] : 0.0f, accumulate);
        }
        return;
    }

    // A: row = lane & 15 (the pixel), k = lane >> 4;  B: k = lane >> 4, column = lane & 15 (the channel)
    const int r = lane & 15, kq = lane >> 4;
    const long m0 = p0 + wave * cm::kTile, p = m0 + r;
    const bool tile_live = m0 < npix, valid = p < npix;                             // (tile_live is uniform in the wave)
    const long pc = valid ? p : npix - 1;
    const int b = (int)(pc / nps), pin = (int)(pc - (long)b * nps), oy = pin / g.OW, ox = pin - oy * g.OW;
    const cm::Band band = cm::band_of(p0, npix, b, g);
    const uint8_t *slot = bands + (b - bfirst) * slot_bytes;
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};
    int ky = 0, kx = 0, cb = 0;                                                     // the round's tap and block of 16 channels
    int off = valid ? cm::tap_offset(g, band, oy, ox, 0, 0) : -1;
    for (int sl = 0; sl < nslab; ++sl) {
        if (sl + 1 < nslab) load_slab(sl + 1);                                      // in flight while this slab feeds the chains
        const float *sb = slab + (sl & 1) * SF + kq * RS + r;
        if (tile_live) {
            // the slab's four rounds, unrolled: their LDS reads do not wait for the chains.  Behind the last tap (a partial last slab) a
            // round is zeros times the slab's zero rows, which leaves the accumulators as they are.
            WideQuad q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                q[j] = {{0u, 0u, 0u, 0u}};
                if (off >= 0) q[j] = *(const WideQuad *)(slot + off + cb * 16);     // (a tap outside the image: zeros, nothing read)
                if (++cb == CPB) {                                                  // (uniform) the next tap
                    cb = 0;
                    if (++kx == g.KW) { kx = 0; ++ky; }
                    off = valid && ky < g.KH ? cm::tap_offset(g, band, oy, ox, ky, kx) : -1;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float a = cm::spike_of(q[j], u, kq);
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sb[(j * 16 + 4 * u) * RS + t * 16], acc[t], 0, 0, 0);
                }
        }
        if (sl + 1 < nslab) store_slab(sl + 1);                                     // (the other buffer: last read before the previous barrier)
        __syncthreads();
    }
    if (!tile_live) return;

    // C/D layout of the 16x16 shapes: column = lane & 15 (channel), row = (lane >> 4) * 4 + reg (pixel).  Partial tiles are masked
    // here only.  Where OH * OW is a multiple of 4 a lane's four pixels are one sample's, 16 bytes apart from nothing: one 16-byte store.
    const long pq = m0 + kq * 4;
    const bool vec = (nps & 3) == 0 && ((uintptr_t)out & 15) == 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int co = c0 + t * 16 + r;
        if (co >= g.Cout || pq >= npix) continue;
        if (vec) {                                                                  // (npix is a multiple of 4 as well: all four exist)
            const int bq = (int)(pq / nps);
            f32x4 *dst = (f32x4 *)(out + ((size_t)bq * g.Cout + co) * nps + (pq - (long)bq * nps));
            f32x4 prev = {0.f, 0.f, 0.f, 0.f}, v;
            if (accumulate) prev = *dst;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) v[reg] = wide_emit(acc[t][reg], bias, co, prev[reg], accumulate);
            *dst = v;
        } else {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const long pp = pq + reg;
                if (pp >= npix) continue;
                const int bq = (int)(pp / nps);
                const size_t at = ((size_t)bq * g.Cout + co) * nps + (pp - (long)bq * nps);
                out[at] = wide_emit(acc[t][reg], bias, co, accumulate ? out[at] : 0.0f, accumulate);
            }
        }
    }
}

struct Plan {
    int rc, NT, OH, OW;
    long long blocks;
    unsigned long long lds;
};

// The number of channel tiles per wave.  More tiles per wave share one A fragment and one band between more chains, but make fewer
// workgroups, and a wave's time grows with its MFMAs: measured (profiles/NOTES_conv_mfma.md) a call at B = 1 and 16 takes 13.5 / 19.6 /
// 29.3 us (32 -> 64) and 20.2 / 30.6 / 47.1 us (64 -> 128) with NT = 1 / 2 / 4 -- a layer of a converted network is small, so the first
// thing is to spread.  NT = 2 won only at B = 128, 32 -> 64 (38.0 against 41.5 us: 1024 workgroups of NT = 2), and lost at 64 -> 128
// (39.8 against 38.3 us: 512); NT = 4 won nowhere and is not instantiated.  The rule: NT = 2 where that still leaves 1024 workgroups,
// four for each of the 256 CUs, else 1.  A group wider than the padded Cout is never taken, nor one whose LDS does not fit.
constexpr long long kSpreadWorkgroups = 1024;

Plan plan_for(int B, int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad) {
    Plan pl = {SNN_ERR_INVALID, 1, 0, 0, 0, 0};
    if (B <= 0 || Cin <= 0 || H <= 0 || Wd <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0) return pl;
    pl.OH = (H + 2 * pad - KH) / stride + 1, pl.OW = (Wd + 2 * pad - KW) / stride + 1;
    if (pl.OH <= 0 || pl.OW <= 0) return pl;
    pl.rc = SNN_ERR_UNSUPPORTED;
    // index widths, as snn_prop_conv2d_f32; here the PADDED term index is an int too
    if ((long long)Cin * KH * KW > SNN_CONV2D_MAX_TAPS || (long long)Cin * H * Wd > SNN_CONV2D_MAX_IMAGE ||
        (long long)pl.OH * pl.OW > SNN_CONV2D_MAX_IMAGE || (long long)cm::padded_channels(Cin) * KH * KW > SNN_CONV2D_MAX_TAPS)
        return pl;
    const WideGeom g = {Cin, H, Wd, KH, KW, stride, pad, pl.OH, pl.OW, Cout};
    if ((unsigned long long)cm::band_rows_max(g) * Wd >= (1ull << 24)) return pl;     // (before its product with the pixel stride is trusted)
    pl.blocks = ((long long)B * pl.OH * pl.OW + cm::kBlockPix - 1) / cm::kBlockPix;
    if (pl.blocks >= (1ll << 24)) return pl;
    const int tiles = (Cout + 15) / 16;
    for (int NT = 2; NT >= 1; NT >>= 1) {
        const long long wgs = pl.blocks * ((tiles + NT - 1) / NT);
        pl.lds = cm::lds_bytes(g, B, NT);
        if (NT > 1 && (NT > tiles || wgs < kSpreadWorkgroups || pl.lds > (unsigned long long)cm::kLdsLimit)) continue;
        // (a grid's threads, workgroups x 256, stay below 2^32)
        if (pl.lds > (unsigned long long)cm::kLdsLimit || wgs * (cm::kWaves * 64) >= (1ll << 32)) return pl;
        pl.NT = NT;
        pl.rc = SNN_OK;
        return pl;
    }
    return pl;
}

template <int NT>
int launch(const Plan &pl, const float *W, const float *bias, const uint8_t *s, float *out, int B, const WideGeom &g, int accumulate,
           int *counters, hipStream_t stream) {
    // beyond 64 KiB a launch needs the attribute; set for every such launch (it belongs to the current device, and costs nothing measurable)
    if (pl.lds > 64 * 1024 &&
        snn_check(hipFuncSetAttribute((const void *)k_conv_mfma<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, cm::kLdsLimit)))
        return SNN_ERR_LAUNCH;
    const int ngroups = ((g.Cout + 15) / 16 + NT - 1) / NT;
    hipLaunchKernelGGL(k_conv_mfma<NT>, dim3((unsigned)(pl.blocks * ngroups)), dim3(cm::kWaves * 64), (size_t)pl.lds, stream, W, bias, s, out,
                       B, g, accumulate, counters, ngroups);
    return snn_check_launch();
}

}  // namespace

// snn_run.hip (feed_conn) and Conv2dConnection's eager compute(): whether a CONV2D connection that asks (snn_conn_prop.prop_auto)
// propagates through snn_prop_conv2d_mfma_f32 -- the shapes snn_prop_conv2d_f32 hands to k_conv_wide (more than 16 input channels, or
// a bank beyond 64 KiB), where the bands fit the LDS.  A fact of the shape and the request, never of the data; touches no device.
extern "C" int snn_conv2d_mfma_takes(int B, int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad, int asked) {
    if (!asked) return 0;
    if (plan_for(B, Cin, H, Wd, Cout, KH, KW, stride, pad).rc != SNN_OK) return 0;
    return (Cin > 16 || sizeof(float) * (size_t)Cout * Cin * KH * KW > 64 * 1024) ? 1 : 0;
}

extern "C" int snn_prop_conv2d_mfma_f32(const float *W, const float *bias, const uint8_t *s, float *out, int B, int Cin, int H, int Wd,
                                        int Cout, int KH, int KW, int stride, int pad, int accumulate, int *counters,
                                        snn_stream_t stream) {
    if (!W || !s || !out) return SNN_ERR_INVALID;
    const Plan pl = plan_for(B, Cin, H, Wd, Cout, KH, KW, stride, pad);
    if (pl.rc != SNN_OK) return pl.rc;
    const WideGeom g = {Cin, H, Wd, KH, KW, stride, pad, pl.OH, pl.OW, Cout};
    if (pl.NT == 2) return launch<2>(pl, W, bias, s, out, B, g, accumulate, counters, (hipStream_t)stream);
    return launch<1>(pl, W, bias, s, out, B, g, accumulate, counters, (hipStream_t)stream);
}
