// snn_run_dense_sif.hip -- a Connection over spike bytes and its SubtractiveResetIFNodes for all T steps of a run in ONE launch
// (snn_run_dense_sif_f32; the layer-major plan of Network.run).  The order, the LDS layouts, the scan's hand-off and why the bits are the
// generic plan's are in snn_run_dense_sif.hpp, whose bodies this kernel calls.
//
// grid.x = samples x panels of 64 targets, the panels of a sample adjacent; 256 threads = 4 waves, wave w the panel's column tile w.
// The GEMM runs with TIME on the rows: per super block of 64 steps a wave carries four accumulator tiles (16 steps x 16 targets each)
// down the sources as four independent unsplit chains -- sixteen MFMAs per round of 16 sources, the four of a weight operand back to
// back, so that a chain's own MFMA latency is covered by the other three.  The sources go in slabs of 64: while slab k feeds the
// chains out of one spike buffer (and one weight slab), slab k + 1 is in flight in registers (one 16-byte piece of spikes and 16
// weights per thread) and is written to the other buffer behind the chains.  One barrier per slab, which also carries the census of
// the spikes just staged.  A panel that fits (run_dense::resident) is staged once, during the first super block, and read for all T.
// Behind a super block's last slab the wave scans its 64 steps in time order in registers (scan_rows, the state handed from lane group
// to lane group by __shfl) and writes the spike bytes straight to the train; no current goes to memory.  A super block whose staged
// rows held a byte above 1 drops its accumulators and takes run_dense::scalar_output from the rows in memory instead.
// No workgroup reads what another writes in the same launch; nothing waits or spins.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_run_dense_sif.hpp"

using namespace snn;
namespace cm = snn::conv_mfma;
namespace rds = snn::run_dense;
namespace da = snn::dense_auto;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = rds::kWaves * 64;
constexpr int kWPer = rds::kSlabK * rds::kPanel / kThreads;                         // weights of a slab per thread

struct RunState {
    float *v, *refrac, *summed, *x;
    uint8_t *s;
};

template <bool RESIDENT>
__global__ __launch_bounds__(kThreads) void k_run_dense_sif(const float *__restrict__ W, const float *__restrict__ bias,
                                                            const uint8_t *__restrict__ s0, const uint8_t *__restrict__ s_train,
                                                            uint8_t *__restrict__ out_train, RunState st, snn_lif_params p, int T, int B,
                                                            int Nin, int N, int npanels) {
    constexpr int WS = rds::kWStride, SS = rds::kSpikeStride, SF = rds::kSlabFloats, SB = rds::kSpikeBytes, NTB = rds::kTimeBlocks;
    extern __shared__ __align__(16) unsigned char rd_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nslab = rds::slabs(Nin), nsuper = (T + rds::kSuper - 1) / rds::kSuper;
    const int c0 = (int)(blockIdx.x % (unsigned)npanels) * rds::kPanel, b = (int)(blockIdx.x / (unsigned)npanels);
    float *wl = (float *)rd_lds;                                                    // RESIDENT: [nslab][kSlabK][WS]; else [2][kSlabK][WS]
    uint8_t *sbuf = rd_lds + (RESIDENT ? rds::panel_bytes(Nin) : 2ull * SF * sizeof(float));      // [2][kSuper][SS]
    const bool whole = (Nin & 15) == 0 && (((uintptr_t)s0 | (uintptr_t)s_train) & 15) == 0;

    // staging: a thread's piece of spikes is 16 sources of step srow of the super block; its weights are column wcol of rows wrow + 4 i
    const int srow = tid >> 2, spiece = (tid & 3) * 16, wcol = tid & 63, wrow = tid >> 6;
    uint32_t sw[4];
    float wr[kWPer];
    da::census cen = {0, 0};
    auto load_spikes = [&](int sb, int sl) __attribute__((always_inline)) {
        rds::stage_piece(s0, s_train, sb * rds::kSuper + srow, T, b, B, Nin, sl * rds::kSlabK + spiece, whole, sw);
    };
    auto store_spikes = [&](uint8_t *dst) __attribute__((always_inline)) {
        *(uint4 *)(dst + srow * SS + spiece) = make_uint4(sw[0], sw[1], sw[2], sw[3]);
        da::census_piece(sw, cen);
    };
    auto load_w = [&](int sl) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kWPer; ++i) wr[i] = rds::panel_weight(W, Nin, N, sl * rds::kSlabK + wrow + 4 * i, c0 + wcol);
    };
    auto store_w = [&](float *dst) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kWPer; ++i) dst[(wrow + 4 * i) * WS + wcol] = wr[i];
    };

    load_spikes(0, 0);
    load_w(0);
    store_spikes(sbuf);
    store_w(wl);
    int flag = __syncthreads_or(cen.above1);                                        // slab 0 of super block 0 holds a byte above 1

    // the wave's tiles: A row = lane & 15 (a step), k = lane >> 4; C column = lane & 15 (target c0 + wave * 16 + r), rows kq * 4 + reg
    const int r = rds::tile_col(lane), kq = lane >> 4;
    const int col = c0 + wave * rds::kTile + r;
    const bool tile_live = c0 + wave * rds::kTile < N, colv = col < N;              // (tile_live is uniform in the wave)
    const size_t n = (size_t)b * N + (colv ? col : 0);
    const bool sums = st.summed != nullptr;
    float v = colv ? st.v[n] : 0.f, rf = colv ? st.refrac[n] : 0.f;
    float sm = colv && sums ? st.summed[n] : 0.f, x = colv && p.traces ? st.x[n] : 0.f;
    const int src = rds::handoff_source(lane);

    f32x4 acc[NTB];
#pragma unroll
    for (int tb = 0; tb < NTB; ++tb) acc[tb] = {0.f, 0.f, 0.f, 0.f};
    unsigned gs = 0;                                                                // slabs walked so far: the buffers' parity
    int dirty = 0;
    for (int sb = 0; sb < nsuper; ++sb) {
        for (int sl = 0; sl < nslab; ++sl) {
            dirty |= flag;
            const bool last = sb + 1 == nsuper && sl + 1 == nslab;
            const int nsl = sl + 1 < nslab ? sl + 1 : 0, nsb = sl + 1 < nslab ? sb : sb + 1;
            const bool wnext = RESIDENT ? (sb == 0 && sl + 1 < nslab) : !last;      // (uniform)
            if (!last) load_spikes(nsb, nsl);
            if (wnext) load_w(nsl);

            {   // (a wave whose column tile is beyond N walks its chain of zero weights too: a branch here would make every load above wait)
                const uint8_t *sp = sbuf + (size_t)(gs & 1u) * SB + r * SS;
                const float *wb = wl + (size_t)(RESIDENT ? sl : (int)(gs & 1u)) * SF + kq * WS + wave * rds::kTile + r;
#pragma unroll
                for (int j = 0; j < rds::kSlabK / 16; ++j) {
                    WideQuad q[NTB];
#pragma unroll
                    for (int tb = 0; tb < NTB; ++tb) q[tb] = *(const WideQuad *)(sp + tb * rds::kTile * SS + j * 16);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float w = wb[(j * 16 + 4 * u) * WS];
#pragma unroll
                        for (int tb = 0; tb < NTB; ++tb)
                            acc[tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(cm::spike_of(q[tb], u, kq), w, acc[tb], 0, 0, 0);
                    }
                }
            }

            cen = {0, 0};
            if (!last) store_spikes(sbuf + (size_t)((gs + 1u) & 1u) * SB);          // (the other buffers: last read before the previous barrier)
            if (wnext) store_w(wl + (size_t)(RESIDENT ? nsl : (int)((gs + 1u) & 1u)) * SF);
            ++gs;
            if (!last) flag = __syncthreads_or(cen.above1);
        }

        // the super block's 64 steps, in time order
        if (tile_live) {
            const int t0 = sb * rds::kSuper;
            if (dirty) {                                                            // (uniform) a byte above 1: the stated order, sum by sum
#pragma unroll 1
                for (int i = 0; i < NTB * 4; ++i) {                                 // (one copy of the body; the result selected into its register)
                    const int t = t0 + (i >> 2) * rds::kTile + rds::tile_row(lane, i & 3);
                    const float a = t < T && colv ? rds::scalar_output(rds::step_row(s0, s_train, t, b, B, Nin), W, Nin, N, col) : 0.f;
#pragma unroll
                    for (int tb = 0; tb < NTB; ++tb)
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) acc[tb][reg] = (tb * 4 + reg == i) ? a : acc[tb][reg];
                }
            }
#pragma unroll
            for (int tb = 0; tb < NTB; ++tb) {
                if (t0 + tb * rds::kTile >= T) break;                               // (uniform; whole time blocks, so the state ends in group 0)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (kq == rds::phase_group(tb * 4 + g) && colv) {
                        const float a[4] = {acc[tb][0], acc[tb][1], acc[tb][2], acc[tb][3]};
                        rds::scan_rows(a, lane, t0 + tb * rds::kTile, T, b, B, N, col, bias, v, rf, sums, sm, x, p, out_train, st.s);
                    }
                    v = __shfl(v, src), rf = __shfl(rf, src), sm = __shfl(sm, src), x = __shfl(x, src);
                }
            }
#pragma unroll
            for (int tb = 0; tb < NTB; ++tb) acc[tb] = {0.f, 0.f, 0.f, 0.f};
        }
        dirty = 0;
    }

    // the state behind step T-1 (scan_rows stored s)
    if (tile_live && kq == 0 && colv) {
        st.v[n] = v;
        st.refrac[n] = rf;
        if (sums) st.summed[n] = sm;
        if (p.traces) st.x[n] = x;
    }
}

struct Plan {
    int rc, resident, npanels;
    long long grid;
    unsigned long long lds;
};

Plan plan_for(int T, int B, int Nin, int N) {
    Plan pl = {SNN_ERR_INVALID, 0, 0, 0, 0};
    if (T <= 0 || B <= 0 || Nin <= 0 || N <= 0) return pl;
    pl.rc = SNN_ERR_UNSUPPORTED;
    if (Nin >= (1 << 24) || B > 65535) return pl;                                   // the int limits of snn_prop_dense_auto_f32
    const long long frames = (long long)T * B;
    if (frames > INT_MAX || frames * N > INT_MAX || frames * Nin > INT_MAX) return pl;
    pl.npanels = (N + rds::kPanel - 1) / rds::kPanel;
    pl.grid = (long long)B * pl.npanels;
    if (pl.grid > INT_MAX) return pl;
    pl.resident = rds::resident(Nin) ? 1 : 0;
    pl.lds = rds::lds_bytes(Nin);
    if (pl.lds > (unsigned long long)cm::kLdsLimit) return pl;
    pl.rc = SNN_OK;
    return pl;
}

template <bool RESIDENT>
int launch(const Plan &pl, const float *W, const float *bias, const uint8_t *s0, const uint8_t *s_train, uint8_t *out_train, const RunState &st,
           const snn_lif_params &p, int T, int B, int Nin, int N, hipStream_t stream) {
    if (pl.lds > 64 * 1024 &&
        snn_check(hipFuncSetAttribute((const void *)k_run_dense_sif<RESIDENT>, hipFuncAttributeMaxDynamicSharedMemorySize, cm::kLdsLimit)))
        return SNN_ERR_LAUNCH;
    hipLaunchKernelGGL(k_run_dense_sif<RESIDENT>, dim3((unsigned)pl.grid), dim3(kThreads), (size_t)pl.lds, stream, W, bias, s0, s_train, out_train,
                       st, p, T, B, Nin, N, pl.npanels);
    return snn_check_launch();
}

}  // namespace

// 0: not taken; 1: taken, the weight panel resident in LDS; 2: taken, the panel streaming.  A fact of the shape; touches no device.
extern "C" int snn_run_dense_sif_takes(int T, int B, int Nin, int N) {
    const Plan pl = plan_for(T, B, Nin, N);
    return pl.rc != SNN_OK ? 0 : pl.resident ? 1 : 2;
}

extern "C" int snn_run_dense_sif_f32(const float *W, const float *bias, const uint8_t *s0, const uint8_t *s_train, uint8_t *out_train, float *v,
                                     float *refrac, float *summed, float *x, uint8_t *s, const snn_lif_params *h_p, int T, int B, int Nin, int N,
                                     snn_stream_t stream) {
    if (!W || !s0 || !out_train || !v || !refrac || !s || !h_p || (T > 1 && !s_train)) return SNN_ERR_INVALID;
    if (h_p->traces && !x) return SNN_ERR_INVALID;
    const Plan pl = plan_for(T, B, Nin, N);
    if (pl.rc != SNN_OK) return pl.rc;
    const RunState st = {v, refrac, summed, x, s};
    if (pl.resident) return launch<true>(pl, W, bias, s0, s_train, out_train, st, *h_p, T, B, Nin, N, (hipStream_t)stream);
    return launch<false>(pl, W, bias, s0, s_train, out_train, st, *h_p, T, B, Nin, N, (hipStream_t)stream);
}
