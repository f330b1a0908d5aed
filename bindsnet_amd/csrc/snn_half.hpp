// snn_half.hpp -- the order- and rounding-carrying bodies of the float16 / bfloat16 Weight features
// (MulticompartmentConnection with one Weight(value_dtype=torch.float16 | torch.bfloat16): bindsnet/network/topology.py:437-479,
// bindsnet/network/topology_features.py:250-266, :633-645, bindsnet/learning/MCC_learning.py:86-110, :224-302).
//
// Only the Weight.value tensor is 2 bytes wide; neuron state, traces and currents stay float32.  Every operation below is float32
// arithmetic on exactly widened values with ONE round-to-nearest-even conversion back ("->h", overflow to +-inf included) wherever
// the reference stores into, or produces, a tensor of the weight dtype (INTEGRATION.md section 3 has the table):
//
//   propagation   (value * spikes).sum(1): the float32 sum in ATen's order over the widened weights (snn_order.hpp OuterSum, a
//                 silent source adds +0 and is not loaded), ->h, widened, stored or added to the float32 current;
//   PostPre       w = (float(w) - pre * dt) ->h   when nu[0] != 0;   w = (float(w) + post * dt) ->h   when nu[1] != 0;
//                 w = (float(w) * decay) ->h      (the Python scalar as float32, not rounded to the weight dtype);
//                 w = clamp(w, min, max) ->h      (clamping in float32 and rounding equals clamping against the rounded bounds:
//                 the rounded bound is the nearest representable value, so no representable w lies between the two);
//                 pre / post are the batch sums of snn_order.hpp batch_sum over the float32 outer products, B = 1 is squeeze;
//   normalise     cs = colsum ->h (zero -> 1);  r = (1 / cs) ->h;  f = (float(r) * norm) ->h;  w = (float(w) * float(f)) ->h
//                 (torch evaluates `norm / abs_sum` on a tensor as abs_sum.reciprocal() * norm).
//
// No packed-half arithmetic anywhere; built with -ffp-contract=off like everything else.  The bodies are __host__ __device__:
// tests/hostcheck/half_host.hip runs them on the CPU against torch (tests/test_half_hostcheck.py).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <string.h>
#include "snn_order.hpp"

namespace snn {

constexpr int kWF32 = 0, kWF16 = 1, kWBF16 = 2;      // snn_conn_desc.w_dtype
constexpr int kHalfMaxB = 256;                       // batch size up to which the PostPre spike masks are kept (8 words)
constexpr int kHalfMaskWords = kHalfMaxB / 32;

__host__ __device__ __forceinline__ float half_bits_to_float(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}
__host__ __device__ __forceinline__ uint32_t half_float_to_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

// float16: the IEEE conversions of hip_fp16.h.  bfloat16: the upper half of the float32 pattern; narrowing rounds to nearest even on
// the discarded 16 bits and turns every NaN into the quiet 0x7FC0 (what c10::BFloat16 does).
template <int DT>
__host__ __device__ __forceinline__ float half_widen(uint16_t h) {
    if (DT == kWF16) return __half2float(__ushort_as_half(h));
    return half_bits_to_float((uint32_t)h << 16);
}
// The value a narrowing starts from is a float32 IN A REGISTER.  Without this the device compiler folds the float32 operation in
// front of a float16 conversion into one 16-bit-result instruction -- (half)(1.0f / float(h)) into v_rcp_f16, (half)(float(h) * x)
// into v_fma_mixlo_f16 --, i.e. an approximate reciprocal, or one rounding of the exact product where the reference rounds to
// float32 first and to float16 after (seen on an MI355X: two columns' normalisation factors one step off).
__host__ __device__ __forceinline__ float half_f32_value(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(f));
#endif
    return f;
}
template <int DT>
__host__ __device__ __forceinline__ uint16_t half_narrow(float f) {
    f = half_f32_value(f);
    if (DT == kWF16) return __half_as_ushort(__float2half_rn(f));
    if (f != f) return (uint16_t)0x7FC0u;
    const uint32_t u = half_float_to_bits(f);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
// one ->h rounding of a float32 value, returned widened again
template <int DT>
__host__ __device__ __forceinline__ float half_round(float f) { return half_widen<DT>(half_narrow<DT>(f)); }

// ---- propagation: what the column's float32 total becomes in the target's current ----------------------------------------
template <int DT>
__host__ __device__ __forceinline__ float half_prop_finish(float total, float before, int accumulate) {
    return (accumulate ? before : 0.0f) + half_round<DT>(total);
}

// ---- PostPre: one element (i, j) of the [Nin, N] value.  mS / mT: bit b of word b / 32 (words `strideS` / `strideT` apart) says
// whether sample b's source neuron i / target neuron j spiked; the sums visit the samples in batch_sum's order and load the
// factors of a sample only where its bit is set (every other term is +0).
struct HalfPostPre {
    const uint8_t *s_src; const float *x_src; const uint8_t *s_tgt; const float *x_tgt;
    int B, Nin, N;
    float nu0, nu1; int use_dt; float dt, decay; int has_min; float wmin; int has_max; float wmax;
};

__host__ __device__ __forceinline__ bool half_mask_any(const uint32_t *m, int stride, int B) {
    uint32_t any = 0;
    for (int w = 0; w < (B + 31) / 32; ++w) any |= m[(size_t)w * stride];
    return any != 0;
}

// R: the batch reduction (snn_order.hpp batch_sum<R>; SUM is the function as it was).  An element without an event keeps u = 0 under each of them.
template <int DT, int R = kReduceSum>
__host__ __device__ inline uint16_t half_postpre_elem(uint16_t wbits, const HalfPostPre &a, int i, int j, const uint32_t *mS, int strideS,
                                                      const uint32_t *mT, int strideT) {
    const long E = (long)a.Nin * a.N, e = (long)i * a.N + j;
    float w = half_widen<DT>(wbits);
    if (a.nu0 != 0.f) {                                  // MCC_learning.py:233-263: sum_b s_src[b,i] * (x_tgt[b,j] * nu0)
        auto term = [&](int b) -> float {
            if (!((mS[(size_t)(b >> 5) * strideS] >> (b & 31)) & 1u)) return 0.f;
            return (float)a.s_src[(size_t)b * a.Nin + i] * (a.x_tgt[(size_t)b * a.N + j] * a.nu0);
        };
        float u = 0.f;
        if (a.B == 1) u = term(0);                       // reduction = torch.squeeze
        else if (half_mask_any(mS, strideS, a.B)) u = batch_sum<R>(term, a.B, e, E);
        if (a.use_dt) u = u * a.dt;
        w = half_round<DT>(w - u);
    }
    if (a.nu1 != 0.f) {                                  // :267-299: sum_b x_src[b,i] * (s_tgt[b,j] * nu1)
        auto term = [&](int b) -> float {
            if (!((mT[(size_t)(b >> 5) * strideT] >> (b & 31)) & 1u)) return 0.f;
            return a.x_src[(size_t)b * a.Nin + i] * ((float)a.s_tgt[(size_t)b * a.N + j] * a.nu1);
        };
        float u = 0.f;
        if (a.B == 1) u = term(0);
        else if (half_mask_any(mT, strideT, a.B)) u = batch_sum<R>(term, a.B, e, E);
        if (a.use_dt) u = u * a.dt;
        w = half_round<DT>(w + u);
    }
    w = half_round<DT>(w * a.decay);                     // :93-94 (decay == 1 multiplies too: exact)
    if (a.has_min && w < a.wmin) w = a.wmin;             // :102-110
    if (a.has_max && w > a.wmax) w = a.wmax;
    return half_narrow<DT>(w);
}

// ---- normalise: column j's scale factor f (widened), and the scaling of one element ----------------------------------------
// The column sum in ATen's sum(dim=0) order (OuterSum: multi_row_sum below 32*floor(N/32), row_sum behind), 16 rows loaded
// ahead of their adds.
template <int DT>
__host__ __device__ inline float half_norm_factor(const uint16_t *W, int Nin, int N, int j, float norm) {
    OuterSum acc;
    acc.init(outer_tail(j, N));
    for (int base = 0; base < Nin; base += 16) {
        uint16_t v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = base + k < Nin ? W[(size_t)(base + k) * N + j] : (uint16_t)0;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (base + k < Nin) acc.add(base + k, half_widen<DT>(v[k]), Nin);
    }
    float cs = half_round<DT>(acc.finish(Nin));          // topology_features.py:262
    if (cs == 0.f) cs = 1.0f;                            // :265
    const float r = half_round<DT>(1.0f / cs);           // `norm / abs_sum` == abs_sum.reciprocal() * norm
    return half_round<DT>(r * norm);
}
template <int DT>
__host__ __device__ __forceinline__ uint16_t half_norm_scale(uint16_t wbits, float f) {
    return half_narrow<DT>(half_widen<DT>(wbits) * f);
}

}  // namespace snn
