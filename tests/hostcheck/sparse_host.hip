// Host-side check of bindsnet_amd/csrc/snn_sparse.hpp: the __host__ __device__ bodies of SparseConnection's propagation -- the
// segment look-up, the ordered walk and the accumulate / finish steps -- are run HERE on the CPU (compiled by hipcc like the kernel,
// no device code is executed), one (column tile, sample) pair at a time, exactly as k_prop_sparse's waves call them: per 1024-source
// chunk the spiking sources ascending, their non-empty segments, then the walk.  A wave's lanes move from one segment to the next
// together, which a CPU loop over lanes does not: with lanes == 1 ONE worker walks the whole segment list (the walk's batching and
// look-ahead as the kernel runs them, a segment's entries one after another); with lanes > 1 the list is handed over one segment at
// a time and every lane takes its entries of it (the kernel's entry <-> lane mapping).  Test infrastructure only
// (tests/test_sparse_hostcheck.py); not part of libsnnhip.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_sparse.hpp"

// out [B, N] (+)= the sparse product of s [B, Nin] 0/1 bytes with the compiled form (ptr, col, val, nnz), + bias (nullable)
extern "C" int hostcheck_sparse_prop(const int *ptr, const uint8_t *col, const float *val, int nnz, const float *bias, const uint8_t *s,
                                     float *out, int B, int Nin, int N, int accumulate, int lanes) {
    const int tiles = (N + snn::kSparseTJ - 1) / snn::kSparseTJ;
    for (int b = 0; b < B; ++b)
        for (int tile = 0; tile < tiles; ++tile) {
            float acc[snn::kSparseTJ];
            for (int c = 0; c < snn::kSparseTJ; ++c) acc[c] = 0.0f;
            for (int base = 0; base < Nin; base += snn::kSparseChunk) {
                std::vector<snn::SparseSeg> segs;
                for (int i = base; i < Nin && i < base + snn::kSparseChunk; ++i) {
                    const uint8_t sv = s[(size_t)b * Nin + i];
                    if (!sv) continue;
                    snn::SparseSeg sg{0, 0, (float)sv};
                    snn::sparse_segment(ptr, tile, Nin, i, nnz, sg.beg, sg.end);
                    if (sg.end > sg.beg) segs.push_back(sg);
                }
                if (lanes == 1) snn::sparse_walk(acc, segs.data(), (int)segs.size(), col, val, 0, 1);
                else
                    for (size_t k = 0; k < segs.size(); ++k)
                        for (int lane = 0; lane < lanes; ++lane) snn::sparse_walk(acc, &segs[k], 1, col, val, lane, lanes);
            }
            for (int c = 0; c < snn::kSparseTJ; ++c) {
                const int j = tile * snn::kSparseTJ + c;
                if (j >= N) break;
                const size_t o = (size_t)b * N + j;
                out[o] = snn::sparse_finish(acc[c], bias, j, accumulate ? out[o] : 0.0f);
            }
        }
    return 0;
}
