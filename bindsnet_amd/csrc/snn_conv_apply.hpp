// snn_conv_apply.hpp -- the batch reduction in phase 2 of the Conv2dConnection outer-product rules (PostPre, Hebbian,
// WeightDependentPostPre; learning.py:457-497, :1348-1380, :920-976): one weight element reduces its per-sample partial sums `part`
// [2][B][E] (pre | post, written by the partial kernels of snn_ops.hip) over the batch; k_conv_pp_apply / k_conv_hebb_apply (snn_ops.hip)
// then apply rates, decay and clamp.  __host__ __device__ so that tests/hostcheck/reduction_host.hip runs the same text on the CPU.
// ACC: OuterSum (ATen's sum(dim=0) order), or the BatchReduce<R> of another reduction (snn_order.hpp) -- every sample is a term here, so
// nothing is folded in.  Built with -ffp-contract=off: every operation below rounds once.
#pragma once
#include "snn_order.hpp"

namespace snn {

// element e's partial sums of the B samples in ATen's sum(dim=0) order (the loads of sixteen samples are issued together, then added in that
// order: one round trip per sixteen terms)
template <class ACC = OuterSum>
__host__ __device__ __forceinline__ float conv_pp_batch_sum(const float *__restrict__ base, int B, long E, long e, bool tail) {
    ACC acc; acc.init(tail);
    for (int b0 = 0; b0 < B; b0 += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = base[(size_t)min(b0 + u, B - 1) * E + e];
#pragma unroll
        for (int u = 0; u < 16; ++u) if (b0 + u < B) acc.add(b0 + u, v[u], B);
    }
    return acc.finish(B);
}

}  // namespace snn
