// The bodies of bindsnet_amd/csrc/snn_run_dense_sif.hpp on the CPU, with k_run_dense_sif's split: sample x panel of 64 targets, super
// blocks of 64 steps, slabs of 64 sources staged through images of the kernel's two LDS regions (stage_piece, panel_weight), the chain
// of a (step, target) as fmaf down the staged slabs, the census and scalar_output, and the scan of a wave's 64 lanes phase by phase
// with the state rotated through handoff_source.  For tests/test_run_dense_sif_hostcheck.py; not in libsnnhip.
#include <algorithm>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_run_dense_sif.hpp"

using namespace snn;
namespace rds = snn::run_dense;
namespace da = snn::dense_auto;

// 0, or -3 for a store outside a staged region; *scalar_blocks counts the super blocks that took the scalar body
extern "C" int hostcheck_run_dense_sif(const float *W, const float *bias, const uint8_t *s0, const uint8_t *s_train, uint8_t *out_train, float *v,
                                       float *refrac, float *summed, float *x, uint8_t *s, int T, int B, int Nin, int N, float thresh,
                                       float refrac_p, int traces, float trace_decay, float trace_scale, int *scalar_blocks) {
    snn_lif_params p = {};
    p.thresh = thresh, p.refrac = refrac_p, p.dt = 1.0f, p.traces = traces, p.trace_decay = trace_decay, p.trace_scale = trace_scale;
    const int nslab = rds::slabs(Nin), nsuper = (T + rds::kSuper - 1) / rds::kSuper, npanels = (N + rds::kPanel - 1) / rds::kPanel;
    const bool whole = (Nin & 15) == 0 && (((uintptr_t)s0 | (uintptr_t)s_train) & 15) == 0;
    if (rds::lds_bytes(Nin) > (unsigned long long)rds::cm::kLdsLimit) return -3;
    std::vector<uint8_t> sp(rds::kSpikeBytes);
    std::vector<float> wl(rds::kSlabFloats), acc(rds::kSuper * rds::kPanel);
    *scalar_blocks = 0;
    for (int b = 0; b < B; ++b)
        for (int panel = 0; panel < npanels; ++panel) {
            const int c0 = panel * rds::kPanel;
            // the lanes' state: every lane of a column starts with the column's state
            float lv[rds::kWaves][64], lr[rds::kWaves][64], lm[rds::kWaves][64], lx[rds::kWaves][64];
            for (int w = 0; w < rds::kWaves; ++w)
                for (int lane = 0; lane < 64; ++lane) {
                    const int col = c0 + w * rds::kTile + rds::tile_col(lane);
                    const size_t n = (size_t)b * N + (col < N ? col : 0);
                    lv[w][lane] = v[n], lr[w][lane] = refrac[n], lm[w][lane] = summed ? summed[n] : 0.f, lx[w][lane] = x ? x[n] : 0.f;
                }
            for (int sb = 0; sb < nsuper; ++sb) {
                const int t0 = sb * rds::kSuper;
                std::fill(acc.begin(), acc.end(), 0.0f);
                da::census cen = {0, 0};
                for (int sl = 0; sl < nslab; ++sl) {
                    for (int tid = 0; tid < rds::kWaves * 64; ++tid) {          // the staging threads
                        uint32_t w4[4];
                        const int srow = tid >> 2, piece = (tid & 3) * 16;
                        rds::stage_piece(s0, s_train, t0 + srow, T, b, B, Nin, sl * rds::kSlabK + piece, whole, w4);
                        if (srow * rds::kSpikeStride + piece + 16 > rds::kSpikeBytes) return -3;
                        memcpy(&sp[srow * rds::kSpikeStride + piece], w4, 16);
                        da::census_piece(w4, cen);
                        for (int i = 0; i < rds::kSlabK / 4; ++i) {
                            const int row = (tid >> 6) + 4 * i, col = tid & 63;
                            if (row * rds::kWStride + col >= rds::kSlabFloats) return -3;
                            wl[row * rds::kWStride + col] = rds::panel_weight(W, Nin, N, sl * rds::kSlabK + row, c0 + col);
                        }
                    }
                    for (int row = 0; row < rds::kSuper; ++row)                  // the chains: one per (step, target), the slab's sources ascending
                        for (int col = 0; col < rds::kPanel; ++col)
                            for (int k = 0; k < rds::kSlabK; ++k)
                                acc[row * rds::kPanel + col] = fmaf((float)sp[row * rds::kSpikeStride + k], wl[k * rds::kWStride + col], acc[row * rds::kPanel + col]);
                }
                if (cen.above1) {
                    ++*scalar_blocks;
                    for (int row = 0; row < rds::kSuper && t0 + row < T; ++row)
                        for (int col = 0; col < rds::kPanel && c0 + col < N; ++col)
                            acc[row * rds::kPanel + col] = rds::scalar_output(rds::step_row(s0, s_train, t0 + row, b, B, Nin), W, Nin, N, c0 + col);
                }
                for (int w = 0; w < rds::kWaves; ++w) {
                    if (c0 + w * rds::kTile >= N) continue;
                    for (int ph = 0; ph < 4 * rds::kTimeBlocks; ++ph) {
                        const int tb = ph >> 2;
                        if (t0 + tb * rds::kTile >= T) break;
                        for (int lane = 0; lane < 64; ++lane) {
                            const int col = c0 + w * rds::kTile + rds::tile_col(lane);
                            if ((lane >> 4) != rds::phase_group(ph) || col >= N) continue;
                            float a[4];
                            for (int reg = 0; reg < 4; ++reg) a[reg] = acc[(tb * rds::kTile + rds::tile_row(lane, reg)) * rds::kPanel + (col - c0)];
                            rds::scan_rows(a, lane, t0 + tb * rds::kTile, T, b, B, N, col, bias, lv[w][lane], lr[w][lane], summed != nullptr, lm[w][lane],
                                           lx[w][lane], p, out_train, s);
                        }
                        float nv[64], nr[64], nm[64], nx[64];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int src = rds::handoff_source(lane);
                            nv[lane] = lv[w][src], nr[lane] = lr[w][src], nm[lane] = lm[w][src], nx[lane] = lx[w][src];
                        }
                        memcpy(lv[w], nv, sizeof nv), memcpy(lr[w], nr, sizeof nr), memcpy(lm[w], nm, sizeof nm), memcpy(lx[w], nx, sizeof nx);
                    }
                }
            }
            for (int w = 0; w < rds::kWaves; ++w)
                for (int lane = 0; lane < 16; ++lane) {                          // group 0 holds the state behind step T-1
                    const int col = c0 + w * rds::kTile + lane;
                    if (col >= N) continue;
                    const size_t n = (size_t)b * N + col;
                    v[n] = lv[w][lane], refrac[n] = lr[w][lane];
                    if (summed) summed[n] = lm[w][lane];
                    if (x) x[n] = lx[w][lane];
                }
        }
    return 0;
}
