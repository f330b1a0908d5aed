// snn_sparse.hip -- SparseConnection.compute on gfx950 (include/snnhip.h, snn_prop_sparse_f32).
//
// grid (ceil(N/256), B), ONE wave of 64 lanes per workgroup: workgroup <-> (column tile, sample).  The tile's 256 running
// sums live in LDS.  Per 1024-source chunk the wave
//   (1) compacts the sample's spiking sources into an ascending list (wave ballot + popcount, as k_prop in snn_ops.hip),
//   (2) looks every listed source's segment of this tile up, 64 sources at a time, and keeps the non-empty ones, order kept,
//   (3) walks those segments in order (snn::sparse_walk): lanes <-> entries of one segment, one segment after another.
// Work is (spiking sources) x (their fan-out); silent sources cost one byte of the spike row each.  The order of the terms
// of one column is the program order of one wave's LDS accesses: no atomics, no barrier between rows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_sparse.hpp"

using namespace snn;

static_assert(kSparseTJ == SNN_SPARSE_TJ, "the tile width is part of the compiled form");

__global__ __launch_bounds__(64) void k_prop_sparse(const int *__restrict__ ptr, const uint8_t *__restrict__ col,
                                                    const float *__restrict__ val, int nnz, const float *__restrict__ bias,
                                                    const uint8_t *__restrict__ s, float *__restrict__ out, int Nin, int N,
                                                    int accumulate) {
    __shared__ float acc[kSparseTJ];
    __shared__ uint32_t list[kSparseChunk];         // (index inside the chunk) << 8 | spike byte, ascending
    __shared__ SparseSeg segs[kSparseChunk];
    const int lane = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const uint8_t *srow = s + (size_t)b * Nin;
    const uint64_t lt = (1ull << lane) - 1ull;
    for (int c = lane; c < kSparseTJ; c += 64) acc[c] = 0.0f;

    for (int base = 0; base < Nin; base += kSparseChunk) {
        uint32_t sv[kSparseChunk / 64];
#pragma unroll
        for (int p = 0; p < kSparseChunk / 64; ++p) {
            const int i = base + p * 64 + lane;
            sv[p] = (i < Nin) ? srow[i] : 0u;
        }
        int n = 0;
#pragma unroll
        for (int p = 0; p < kSparseChunk / 64; ++p) {
            const uint64_t m = __ballot(sv[p] != 0);
            if (sv[p]) list[n + __popcll(m & lt)] = ((uint32_t)(p * 64 + lane) << 8) | sv[p];
            n += __popcll(m);
        }
        __syncthreads();
        int n2 = 0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            SparseSeg sg{0, 0, 0.f};
            if (k < n) {
                const uint32_t e = list[k];
                sparse_segment(ptr, tile, Nin, base + (int)(e >> 8), nnz, sg.beg, sg.end);
                sg.f = (float)(e & 255u);
            }
            const bool have = sg.end > sg.beg;
            const uint64_t m = __ballot(have);
            if (have) segs[n2 + __popcll(m & lt)] = sg;
            n2 += __popcll(m);
        }
        __syncthreads();
        sparse_walk(acc, segs, n2, col, val, lane, 64);
        __syncthreads();
    }
    for (int c = lane; c < kSparseTJ; c += 64) {
        const int j = tile * kSparseTJ + c;
        if (j < N) {
            const size_t o = (size_t)b * N + j;
            out[o] = sparse_finish(acc[c], bias, j, accumulate ? out[o] : 0.0f);
        }
    }
}

extern "C" int snn_prop_sparse_f32(const int *ptr, const uint8_t *col, const float *val, int nnz, const float *bias,
                                   const uint8_t *s, float *out, int B, int Nin, int N, int accumulate, snn_stream_t stream) {
    if (!ptr || !s || !out || B <= 0 || Nin <= 0 || N <= 0 || nnz < 0 || (nnz > 0 && (!col || !val))) return SNN_ERR_INVALID;
    const long long tiles = ((long long)N + kSparseTJ - 1) / kSparseTJ;
    if (B > 65535 || Nin > (1 << 24) || tiles * (long long)Nin + 1 > 2147483647ll) return SNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_prop_sparse, dim3((unsigned)tiles, B), dim3(64), 0, (hipStream_t)stream, ptr, col, val, nnz, bias, s, out,
                       Nin, N, accumulate);
    return snn_check_launch();
}
