// snn_sparse.hpp -- the order-carrying bodies of SparseConnection.compute (bindsnet/network/topology.py:2009-2017 +
// :332-346: `s.view(B, -1).float() @ w (+ b)` with `w` a sparse COO tensor).
//
// Order contract (established against the reference's torch, 1 and 8 threads, DESIGN.md "Summation order"):
//   out[b, j] = (...((0 + w[i1, j]) + w[i2, j]) + ...) + bias[j]
// over the STORED entries of column j whose source i spiked, i ascending, one rounded f32 add per term, the bias last.
// A spike byte enters as float(s) * w, one rounded multiply before the add; the contract is pinned against the reference
// for spike bytes 0/1 and finite weights (a silent source's row is skipped, i.e. its terms are taken as +-0).
//
// Compiled form: a column-tiled CSR.  The N target columns are cut into tiles of SNN_SPARSE_TJ = 256; the stored entries
// are laid out tile by tile, inside a tile by (source i, target j) ascending:
//   ptr [ceil(N/256) * Nin + 1] int32   entries of (tile t, source i) are [ptr[t*Nin + i], ptr[t*Nin + i + 1])
//   col [nnz] uint8                     the entry's column inside its tile (j - 256 t)
//   val [nnz] float32                   its weight
// One worker group (a wave of 64 lanes on the device) owns one (tile, sample) pair and the tile's 256 running sums.  It
// takes the sample's spiking sources in ascending order; the entries of one source's segment go to the lanes (entry e to
// lane (e - beg) % 64).  The columns inside one segment are distinct, so lanes never meet inside a row, and rows follow one
// another in program order, so every column sees its terms in ascending i without atomics.
//
// The bodies are __host__ __device__: tests/hostcheck/sparse_host.hip runs them on the CPU against reference fixtures and
// against torch's own sparse product (tests/test_sparse_hostcheck.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snn {

constexpr int kSparseTJ = 256;          // == SNN_SPARSE_TJ (include/snnhip.h); col is a uint8 because of it
constexpr int kSparseChunk = 1024;      // sources whose spikes are compacted at a time

// One spiking source's entries in one tile: [beg, end) of col / val, f = float(spike byte).
struct SparseSeg { int beg, end; float f; };

// Bounds of (tile, source i), clamped into [0, nnz] so that a table that does not belong to col / val cannot send a read
// outside them.
__host__ __device__ __forceinline__ void sparse_segment(const int *ptr, int tile, int Nin, int i, int nnz, int &beg, int &end) {
    const size_t r = (size_t)tile * (size_t)Nin + (size_t)i;
    int b = ptr[r], e = ptr[r + 1];
    b = b < 0 ? 0 : (b > nnz ? nnz : b);
    e = e < b ? b : (e > nnz ? nnz : e);
    beg = b; end = e;
}

// The accumulate step: one stored entry of a spiking source into its column's running sum.
__host__ __device__ __forceinline__ void sparse_accumulate(float *acc, int c, float f, float w) {
    const float t = f * w;              // float(s) * w
    acc[c] = acc[c] + t;
}

// The walk: segments 0 .. n-1 (ascending source) in order, as worker `lane` of `lanes` sees them -- entries beg + lane,
// beg + lane + lanes, ...  The first entry of the next four segments is fetched before the current four are accumulated
// (on the device the accumulation then waits for its own loads only: s_waitcnt vmcnt(8) in the ISA).
__host__ __device__ inline void sparse_walk(float *acc, const SparseSeg *segs, int n, const uint8_t *col, const float *val, int lane,
                                            int lanes) {
    constexpr int U = 4;
    SparseSeg cs[U], ns[U];
    int cc[U], nc[U];
    float cw[U], nw[U];
    auto fetch = [&](int k0, SparseSeg *sg, int *c, float *w) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k0 + u < n) sg[u] = segs[k0 + u];
            else sg[u] = SparseSeg{0, 0, 0.f};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {       // unconditional loads (a worker without an entry re-reads the segment's first; a
            const int e = sg[u].beg + lane; // segment past the end reads entry 0, which exists because n > 0): no branch between
            const int ee = e < sg[u].end ? e : sg[u].beg;          // the loads, so they can stay in flight across the accumulation
            c[u] = col[ee]; w[u] = val[ee];
        }
    };
    if (n <= 0) return;
    fetch(0, cs, cc, cw);
    for (int k0 = 0; k0 < n; k0 += U) {
        fetch(k0 + U, ns, nc, nw);              // (past the end: empty segments, whose loads are never used)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (cs[u].beg + lane < cs[u].end) sparse_accumulate(acc, cc[u], cs[u].f, cw[u]);
            for (int e = cs[u].beg + lane + lanes; e < cs[u].end; e += lanes) sparse_accumulate(acc, col[e], cs[u].f, val[e]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { cs[u] = ns[u]; cc[u] = nc[u]; cw[u] = nw[u]; }
    }
}

// What a column's running sum becomes in `out`: + bias (nullable), then onto 0 or onto what `out` holds (accumulate).
__host__ __device__ __forceinline__ float sparse_finish(float acc, const float *bias, int j, float prev) {
    float r = acc;
    if (bias) r = r + bias[j];
    return prev + r;
}

}  // namespace snn
