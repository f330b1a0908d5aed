// snn_run_conv_sif.hip -- a Conv2dConnection over spike bytes and its SubtractiveResetIFNodes for all T steps of a run in ONE launch
// (snn_run_conv2d_sif_f32; the layer-major plan of Network.run).  The order, the LDS layouts and why the bits are the generic plan's are
// in snn_run_conv_sif.hpp and snn_conv_mfma.hpp, whose bodies this kernel calls.
//
// grid.x = samples x (blocks of 64 consecutive output pixels of the sample) x (groups of 16 output channels), the groups of a block
// adjacent; 256 threads = 4 waves.  Wave w owns the block's pixel tile w (16 pixels) x the group's 16 channels for the whole run: its
// neurons' v, refrac_count, summed and x are 4 values per lane each, in the C layout of v_mfma_f32_16x16x4_f32 (column = lane & 15 the
// channel, row = (lane >> 4) * 4 + reg the pixel), loaded before step 0 and stored behind step T-1.  Per step the accumulator starts at
// +0, walks conv_mfma's tap order as one unsplit chain, and the step's current reaches v through neuron_step only.
// Weights: a bank that fits (run_conv::resident) is transposed into LDS once and read for all T without a barrier inside a step; a larger
// one streams through two slabs every step as in k_conv_mfma, the buffer's parity running on across the steps.
// Spikes: frame t + 1's band is loaded into registers (kStageRegs words per thread; what is beyond follows behind the chains) while frame
// t feeds the chains, and is written to the other band buffer behind them.  One barrier per step, which also carries the census of the
// frame just staged: a frame with a byte above 1 is computed with conv_mfma::scalar_output in the same register layout.
// Epilogue: a lane's four spikes are four consecutive pixels of one channel, i.e. four consecutive bytes of the output row -- one packed
// 4-byte store per lane, the four lanes of a channel making a 16-byte run, with no trip through LDS (byte stores where OH * OW is no
// multiple of 4).
// No workgroup reads what another writes in the same launch; nothing waits or spins.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_run_conv_sif.hpp"

using namespace snn;
namespace cm = snn::conv_mfma;
namespace rcs = snn::run_conv;
namespace da = snn::dense_auto;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = cm::kWaves * 64;

struct RunState {
    float *v, *refrac, *summed, *x;
    uint8_t *s;
};

template <bool RESIDENT>
__global__ __launch_bounds__(kThreads) void k_run_conv_sif(const float *__restrict__ W, const float *__restrict__ bias,
                                                           const uint8_t *__restrict__ s0, const uint8_t *__restrict__ s_train,
                                                           uint8_t *__restrict__ out_train, RunState st, snn_lif_params p, int T, int B,
                                                           WideGeom g, int ngroups, int nblocks) {
    constexpr int RS = cm::slab_stride(1), SF = cm::slab_floats(1), PER = cm::kSlabRows * 16 / kThreads;
    extern __shared__ __align__(16) unsigned char rc_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nps = g.OH * g.OW, nslab = rcs::slabs(g), CPB = cm::padded_channels(g.Cin) / 16;
    const int c0 = (int)(blockIdx.x % (unsigned)ngroups) * 16;
    const int blk = (int)((blockIdx.x / (unsigned)ngroups) % (unsigned)nblocks), b = (int)(blockIdx.x / ((unsigned)ngroups * nblocks));
    const int p0 = blk * cm::kBlockPix;
    const size_t img = (size_t)g.Cin * g.H * g.Wd, frame = (size_t)B * img;
    float *wl = (float *)rc_lds;                                                    // RESIDENT: [nslab][kSlabRows][RS]; else [2][kSlabRows][RS]
    const unsigned long long wbytes = RESIDENT ? rcs::bank_bytes(g) : 2ull * SF * sizeof(float);
    const unsigned long long bslot = rcs::bands_bytes(g) / 2;
    uint8_t *bands = rc_lds + wbytes;                                               // [2][bslot]
    const cm::Band band = rcs::block_band(p0, g);
    const int nwords = rcs::band_words(g, band);

    float wr[PER];
    auto load_slab = [&](int sl) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const cm::SlabSlot e = cm::slab_slot(tid + i * kThreads);
            wr[i] = cm::slab_weight(W, g, (long long)sl * cm::kSlabRows + e.row, c0 + e.col);
        }
    };
    auto store_slab = [&](float *dst) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const cm::SlabSlot e = cm::slab_slot(tid + i * kThreads);
            dst[e.row * RS + e.col] = wr[i];
        }
    };

    // the start frame's band, and the weights (all slabs, or slab 0)
    da::census cen = {0, 0};
    {
        const uint8_t *sp = s0 + (size_t)b * img;
        uint32_t *dst = (uint32_t *)bands;
        for (int k = tid; k < nwords; k += kThreads) {
            const uint32_t w = rcs::band_word(sp, g, band, k);
            dst[rcs::band_word_slot(g, band, k)] = w;
            da::census_word(w, cen);
        }
    }
    for (int sl = 0; sl < (RESIDENT ? nslab : 1); ++sl) {
        load_slab(sl);
        store_slab(wl + (size_t)sl * SF);
    }
    int scalar = __syncthreads_or(cen.above1);

    // the wave's tile: A row = lane & 15 (pixel m0 + r), k = lane >> 4; C column = lane & 15 (channel c0 + r), rows (lane >> 4) * 4 + reg
    const int r = lane & 15, kq = lane >> 4;
    const int m0 = p0 + wave * cm::kTile, pa = m0 + r;
    const bool tile_live = m0 < nps, valid = pa < nps;                              // (tile_live is uniform in the wave)
    const int pac = valid ? pa : nps - 1, oy = pac / g.OW, ox = pac - oy * g.OW;
    const int pq = m0 + kq * 4, co = c0 + r;                                        // the lane's four neurons: pixels pq .. pq + 3 of channel co
    const bool mine = co < g.Cout && pq < nps;
    const size_t n0 = mine ? ((size_t)b * g.Cout + co) * nps + pq : 0;              // ... at n0 .. n0 + 3 of [B, Cout, OH, OW]
    const int nlive = mine ? (nps - pq < 4 ? nps - pq : 4) : 0;
    const size_t out_frame = (size_t)B * g.Cout * nps;
    const bool sums = st.summed != nullptr;
    const bool packed = (nps & 3) == 0 && (((uintptr_t)out_train | (uintptr_t)st.s) & 3) == 0;

    float v[4], rf[4], sm[4], x[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const bool on = reg < nlive;
        v[reg] = on ? st.v[n0 + reg] : 0.f;
        rf[reg] = on ? st.refrac[n0 + reg] : 0.f;
        sm[reg] = on && st.summed ? st.summed[n0 + reg] : 0.f;
        x[reg] = on && p.traces ? st.x[n0 + reg] : 0.f;
    }

    unsigned gs = 0;                                                                // slabs walked so far: the streaming buffer's parity
    uint32_t spikes = 0;
    for (int t = 0; t < T; ++t) {
        const uint8_t *slot = bands + (size_t)(t & 1) * bslot;
        uint32_t *nslot = (uint32_t *)(bands + (size_t)((t + 1) & 1) * bslot);
        const bool more = t + 1 < T;
        const uint8_t *spn = s_train + (size_t)t * frame + (size_t)b * img;         // frame t: the input of step t + 1 (read only if `more`)
        // frame t + 1's first words: in flight while this frame is computed
        uint32_t sw[rcs::kStageRegs];
        if (more) {
#pragma unroll
            for (int i = 0; i < rcs::kStageRegs; ++i) {
                const int k = tid + i * kThreads;
                sw[i] = k < nwords ? rcs::band_word(spn, g, band, k) : 0u;
            }
        }

        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (scalar) {                                                               // (uniform) a byte above 1: the stated order, neuron by neuron
#pragma unroll 1
            for (int reg = 0; reg < nlive; ++reg) {                                 // (one copy of the body; the result selected into its register)
                const int pp = pq + reg, py = pp / g.OW;
                const float a = cm::scalar_output(slot, band, g, py, pp - py * g.OW, W, co);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = q == reg ? a : acc[q];
            }
        } else {
            int ky = 0, kx = 0, cb = 0;
            int off = valid ? cm::tap_offset(g, band, oy, ox, 0, 0) : -1;
            for (int sl = 0; sl < nslab; ++sl) {
                const bool next = !RESIDENT && (sl + 1 < nslab || more);            // the slab behind this one: the next step's slab 0 at the end
                if (next) load_slab(sl + 1 < nslab ? sl + 1 : 0);
                const float *sb = wl + (size_t)(RESIDENT ? sl : (int)(gs & 1u)) * SF + kq * RS + r;
                if (tile_live) {
                    WideQuad q[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        q[j] = {{0u, 0u, 0u, 0u}};
                        if (off >= 0) q[j] = *(const WideQuad *)(slot + off + cb * 16);
                        if (++cb == CPB) {
                            cb = 0;
                            if (++kx == g.KW) { kx = 0; ++ky; }
                            off = valid && ky < g.KH ? cm::tap_offset(g, band, oy, ox, ky, kx) : -1;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(cm::spike_of(q[j], u, kq), sb[(j * 16 + 4 * u) * RS], acc, 0, 0, 0);
                }
                if (!RESIDENT) {
                    if (next) store_slab(wl + (size_t)((gs + 1u) & 1u) * SF);       // (the other buffer: last read before the previous barrier)
                    ++gs;
                    if (sl + 1 < nslab) __syncthreads();                            // (the step's last slab: the step's own barrier below)
                }
            }
        }

        // the step of the lane's four neurons
        spikes = 0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            if (reg < nlive)
                spikes |= (uint32_t)rcs::neuron_step(acc[reg], bias, co, v[reg], rf[reg], sums, sm[reg], x[reg], p) << (8 * reg);
        if (mine) {
            uint8_t *dst = out_train + (size_t)t * out_frame + n0;
            if (packed) *(uint32_t *)dst = spikes;                                  // (nps a multiple of 4: all four exist, n0 a multiple of 4)
            else
                for (int reg = 0; reg < nlive; ++reg) dst[reg] = (uint8_t)(spikes >> (8 * reg));
        }

        if (more) {                                                                 // frame t + 1 into the other buffer, and its census
            cen = {0, 0};
#pragma unroll
            for (int i = 0; i < rcs::kStageRegs; ++i) {
                const int k = tid + i * kThreads;
                if (k < nwords) {
                    nslot[rcs::band_word_slot(g, band, k)] = sw[i];
                    da::census_word(sw[i], cen);
                }
            }
            for (int k = tid + rcs::kStageRegs * kThreads; k < nwords; k += kThreads) {
                const uint32_t w = rcs::band_word(spn, g, band, k);
                nslot[rcs::band_word_slot(g, band, k)] = w;
                da::census_word(w, cen);
            }
            scalar = __syncthreads_or(cen.above1);
        }
    }

    // the state behind step T-1
    if (mine) {
        if (packed) *(uint32_t *)(st.s + n0) = spikes;
        else
            for (int reg = 0; reg < nlive; ++reg) st.s[n0 + reg] = (uint8_t)(spikes >> (8 * reg));
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            if (reg < nlive) {
                st.v[n0 + reg] = v[reg];
                st.refrac[n0 + reg] = rf[reg];
                if (st.summed) st.summed[n0 + reg] = sm[reg];
                if (p.traces) st.x[n0 + reg] = x[reg];
            }
    }
}

struct Plan {
    int rc, OH, OW, resident;
    long long grid;
    int ngroups, nblocks;
    unsigned long long lds;
};

Plan plan_for(int T, int B, int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad) {
    Plan pl = {SNN_ERR_INVALID, 0, 0, 0, 0, 0, 0, 0};
    if (T <= 0 || B <= 0 || Cin <= 0 || H <= 0 || Wd <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0) return pl;
    pl.OH = (H + 2 * pad - KH) / stride + 1, pl.OW = (Wd + 2 * pad - KW) / stride + 1;
    if (pl.OH <= 0 || pl.OW <= 0) return pl;
    pl.rc = SNN_ERR_UNSUPPORTED;
    // the int limits of snn_prop_conv2d_mfma_f32
    if ((long long)Cin * KH * KW > SNN_CONV2D_MAX_TAPS || (long long)Cin * H * Wd > SNN_CONV2D_MAX_IMAGE ||
        (long long)pl.OH * pl.OW > SNN_CONV2D_MAX_IMAGE || (long long)cm::padded_channels(Cin) * KH * KW > SNN_CONV2D_MAX_TAPS)
        return pl;
    const WideGeom g = {Cin, H, Wd, KH, KW, stride, pad, pl.OH, pl.OW, Cout};
    if ((unsigned long long)cm::band_rows_max(g) * Wd >= (1ull << 24)) return pl;
    pl.nblocks = (pl.OH * pl.OW + cm::kBlockPix - 1) / cm::kBlockPix;
    pl.ngroups = (Cout + 15) / 16;
    pl.grid = (long long)B * pl.nblocks * pl.ngroups;
    if (pl.grid * kThreads >= (1ll << 32)) return pl;
    pl.resident = rcs::resident(g) ? 1 : 0;
    pl.lds = rcs::lds_bytes(g);
    if (pl.lds > (unsigned long long)cm::kLdsLimit) return pl;
    pl.rc = SNN_OK;
    return pl;
}

template <bool RESIDENT>
int launch(const Plan &pl, const float *W, const float *bias, const uint8_t *s0, const uint8_t *s_train, uint8_t *out_train, const RunState &st,
           const snn_lif_params &p, int T, int B, const WideGeom &g, hipStream_t stream) {
    if (pl.lds > 64 * 1024 &&
        snn_check(hipFuncSetAttribute((const void *)k_run_conv_sif<RESIDENT>, hipFuncAttributeMaxDynamicSharedMemorySize, cm::kLdsLimit)))
        return SNN_ERR_LAUNCH;
    hipLaunchKernelGGL(k_run_conv_sif<RESIDENT>, dim3((unsigned)pl.grid), dim3(kThreads), (size_t)pl.lds, stream, W, bias, s0, s_train, out_train,
                       st, p, T, B, g, pl.ngroups, pl.nblocks);
    return snn_check_launch();
}

}  // namespace

// 0: not taken; 1: taken, the bank resident in LDS; 2: taken, the bank streaming.  A fact of the shape; touches no device.
extern "C" int snn_run_conv2d_sif_takes(int T, int B, int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad) {
    const Plan pl = plan_for(T, B, Cin, H, Wd, Cout, KH, KW, stride, pad);
    return pl.rc != SNN_OK ? 0 : pl.resident ? 1 : 2;
}

extern "C" int snn_run_conv2d_sif_f32(const float *W, const float *bias, const uint8_t *s0, const uint8_t *s_train, uint8_t *out_train,
                                      float *v, float *refrac, float *summed, float *x, uint8_t *s, const snn_lif_params *h_p, int T, int B,
                                      int Cin, int H, int Wd, int Cout, int KH, int KW, int stride, int pad, snn_stream_t stream) {
    if (!W || !s0 || !out_train || !v || !refrac || !s || !h_p || (T > 1 && !s_train)) return SNN_ERR_INVALID;
    if (h_p->traces && !x) return SNN_ERR_INVALID;
    const Plan pl = plan_for(T, B, Cin, H, Wd, Cout, KH, KW, stride, pad);
    if (pl.rc != SNN_OK) return pl.rc;
    const WideGeom g = {Cin, H, Wd, KH, KW, stride, pad, pl.OH, pl.OW, Cout};
    const RunState st = {v, refrac, summed, x, s};
    if (pl.resident) return launch<true>(pl, W, bias, s0, s_train, out_train, st, *h_p, T, B, g, (hipStream_t)stream);
    return launch<false>(pl, W, bias, s0, s_train, out_train, st, *h_p, T, B, g, (hipStream_t)stream);
}
