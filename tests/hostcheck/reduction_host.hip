// Host-side check of the batch reductions beside sum (include/snnhip.h f15): the __host__ __device__ bodies the update kernels run --
// BatchReduce<R> / batch_sum<R> (csrc/snn_order.hpp), the per-element finishes of csrc/snn_synparams.hpp, avg_postpre_elem<R> /
// avg_mstdp_elem<R> (csrc/snn_average.hpp), half_postpre_elem<DT, R> (csrc/snn_half.hpp) -- are run HERE on the CPU (compiled by hipcc
// like the kernels, no device code is executed), element by element as the kernels' threads run them.  The dense kernel itself
// (k_plasticity_red, csrc/snn_plasticity.inc) is a __global__ function over LDS tiles; dense_all() below restates its per-element
// statements around the same accumulator and finish bodies, walking only the samples with an event as the kernel's bit masks do, with
// scalar or per-synapse constants.  conv_apply_all(), local_all() and convnd_all() do the same for k_conv_pp_apply / k_conv_hebb_apply
// (around conv_pp_batch_sum<ACC>, csrc/snn_conv_apply.hpp), k_local_postpre and k_convnd_postpre (around batch_sum<R> and the element
// sums of csrc/snn_convnd.hpp).
// Test infrastructure only (tests/test_reduction_hostcheck.py); not part of libsnnhip.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_average.hpp"
#include "../../bindsnet_amd/csrc/snn_conv_apply.hpp"
#include "../../bindsnet_amd/csrc/snn_convnd.hpp"
#include "../../bindsnet_amd/csrc/snn_half.hpp"
#include "../../bindsnet_amd/csrc/snn_synparams.hpp"

using namespace snn;

// out [E] = reduction R over b of terms [B, E], every sample visited (the kernels of snn_local.hip, snn_convnd.hip, snn_half.hpp, snn_average.hpp)
template <int R>
static void reduce_all(const float *terms, int B, long E, float *out) {
    for (long e = 0; e < E; ++e) out[e] = batch_sum<R>([terms, E, e](int b) { return terms[(long)b * E + e]; }, B, e, E);
}

// ... and only the samples with visit [B, E] != 0 added, through the accumulator the dense and conv2d kernels instantiate (the column class
// is theirs: e >= 32 * floor(E / 32) is a row_sum column)
template <int R>
static void reduce_events(const float *terms, const uint8_t *visit, int B, long E, float *out) {
    for (long e = 0; e < E; ++e) {
        BatchReduce<R> acc;
        acc.init(e >= (E / 32) * 32);
        for (int b = 0; b < B; ++b)
            if (visit[(long)b * E + e]) acc.add(b, terms[(long)b * E + e], B);
        out[e] = acc.finish(B);
    }
}

#define DISPATCH(fn, ...)                                          \
    switch (reduce) {                                              \
        case SNN_REDUCE_SUM: fn<kReduceSum>(__VA_ARGS__); break;   \
        case SNN_REDUCE_MEAN: fn<kReduceMean>(__VA_ARGS__); break; \
        case SNN_REDUCE_AMAX: fn<kReduceAmax>(__VA_ARGS__); break; \
        case SNN_REDUCE_AMIN: fn<kReduceAmin>(__VA_ARGS__); break; \
        default: return -1;                                        \
    }

extern "C" int hostcheck_reduce_all(const float *terms, int B, long E, int reduce, float *out) {
    DISPATCH(reduce_all, terms, B, E, out)
    return 0;
}

extern "C" int hostcheck_reduce_events(const float *terms, const uint8_t *visit, int B, long E, int reduce, float *out) {
    DISPATCH(reduce_events, terms, visit, B, E, out)
    return 0;
}

// ---- the dense kernel's element (modes as StdpArgs.mode: 0 PostPre, 1 MSTDP, 2 Hebbian, 3 WeightDependentPostPre), scalar constants ----
struct DenseArgs {
    const uint8_t *s_src; const float *x_src; const uint8_t *s_tgt; const float *x_tgt;     // MSTDP: previous spikes, p_plus, p_minus
    int B, Nin, N, mode;
    float nu0, nu1; int use_dt; float dt, decay; int has_min; float wmin; int has_max; float wmax;
    float reward; const float *reward_vec;
    const snn_synparams *sp;                 // NULL: scalar constants
};

template <int R>
static void dense_all(float *W, DenseArgs a) {
    const long E = (long)a.Nin * a.N;
    const snn_synparams q = a.sp ? *a.sp : snn_synparams{};
    if (a.mode != 1) {                       // (syn_rates of snn_ops.hip: a rate given as a tensor leaves "any entry non-zero" in its place)
        if (q.nu0) a.nu0 = q.nu0_any ? 1.f : 0.f;
        if (q.nu1) a.nu1 = q.nu1_any ? 1.f : 0.f;
    }
    for (long e = 0; e < E; ++e) {
        const int i = (int)(e / a.N), j = (int)(e - (long)i * a.N);
        const bool tail = e >= (E / 32) * 32;
        const SynElem c = syn_elem(q, a.nu0, a.nu1, a.has_min, a.wmin, a.has_max, a.wmax, i, j);
        float w = W[e];
        auto vS = [&](int b) { return a.s_src[(long)b * a.Nin + i]; };
        auto vT = [&](int b) { return a.s_tgt[(long)b * a.N + j]; };
        auto xs = [&](int b) { return a.x_src[(long)b * a.Nin + i]; };
        auto xt = [&](int b) { return a.x_tgt[(long)b * a.N + j]; };
        if (a.mode == 0) {
            if (a.nu0 != 0.f) {
                BatchReduce<R> acc; acc.init(tail);
                for (int b = 0; b < a.B; ++b) if (vS(b)) acc.add(b, (float)vS(b) * (xt(b) * syn_at(q.nu0, 0, q.nu0_cs, a.nu0, 0, j)), a.B);
                w = syn_postpre(w, true, acc.finish(a.B), false, 0.f, a.use_dt, a.dt);
            }
            if (a.nu1 != 0.f) {
                BatchReduce<R> acc; acc.init(tail);
                for (int b = 0; b < a.B; ++b) if (vT(b)) acc.add(b, xs(b) * ((float)vT(b) * c.nu1), a.B);
                w = syn_postpre(w, false, 0.f, true, acc.finish(a.B), a.use_dt, a.dt);
            }
        } else if (a.mode == 2 || a.mode == 3) {
            BatchReduce<R> a1, a2; a1.init(tail); a2.init(tail);
            for (int b = 0; b < a.B; ++b) if (vS(b)) a1.add(b, (float)vS(b) * xt(b), a.B);
            for (int b = 0; b < a.B; ++b) if (vT(b)) a2.add(b, xs(b) * (float)vT(b), a.B);
            const float u1 = a1.finish(a.B), u2 = a2.finish(a.B);
            w = a.mode == 2 ? syn_hebbian(w, u1, u2, c.nu0, c.nu1) : syn_wdpostpre(w, a.nu0 != 0.f, u1, a.nu1 != 0.f, u2, c.nu0, c.nu1, c.lo, c.hi);
        } else {
            BatchReduce<R> acc; acc.init(tail);
            for (int b = 0; b < a.B; ++b) {
                if (!vS(b) && !vT(b)) continue;
                const float el = xs(b) * (float)vT(b) + (float)vS(b) * xt(b);
                acc.add(b, (a.reward_vec ? a.reward_vec[b] : a.reward) * el, a.B);
            }
            w = syn_mstdp(w, acc.finish(a.B), c.nu0);
        }
        W[e] = syn_finish(w, a.decay, c.lo, c.hi);
    }
}

extern "C" int hostcheck_dense_update(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B, int Nin,
                                      int N, int mode, float nu0, float nu1, int use_dt, float dt, float decay, int has_min, float wmin,
                                      int has_max, float wmax, float reward, const float *reward_vec, const snn_synparams *sp, int reduce) {
    const DenseArgs a{s_src, x_src, s_tgt, x_tgt, B, Nin, N, mode, nu0, nu1, use_dt, dt, decay, has_min, wmin, has_max, wmax, reward, reward_vec, sp};
    DISPATCH(dense_all, W, a)
    return 0;
}

// ---- the averaged MCC rules: the reduced update goes into the ring slot ------------------------------------------------------------
template <int R>
static void avg_postpre_all(float *W, const AvgPostPre &a) {
    for (long e = 0; e < (long)a.Nin * a.N; ++e) avg_postpre_elem<R>(W, a, e);
}
template <int R>
static void avg_mstdp_all(float *W, const AvgMstdp &a) {
    for (long e = 0; e < (long)a.Nin * a.N; ++e) avg_mstdp_elem<R>(W, a, e);
}

extern "C" int hostcheck_avg_postpre_red(float *W, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                                         int Nin, int N, float nu0, float nu1, float dt, float decay, int has_min, float wmin, int has_max,
                                         float wmax, int squeeze, float *ring_pre, float *ring_post, int K, int continuous, int idx_pre,
                                         int idx_post, int reduce) {
    if (K < 1 || K > kAvgMaxTerms || idx_pre < 0 || idx_pre >= K || idx_post < 0 || idx_post >= K) return -1;
    AvgPostPre a;
    a.s_src = s_src; a.x_src = x_src; a.s_tgt = s_tgt; a.x_tgt = x_tgt;
    a.B = B; a.Nin = Nin; a.N = N;
    a.nu0 = nu0; a.nu1 = nu1; a.dt = dt; a.squeeze = squeeze;
    a.fin = AvgBounds{decay, has_min, wmin, has_max, wmax};
    a.pre = avg_ring(ring_pre, K, idx_pre, continuous);
    a.post = avg_ring(ring_post, K, idx_post, continuous);
    DISPATCH(avg_postpre_all, W, a)
    return 0;
}

extern "C" int hostcheck_avg_mstdp_red(float *W, float *p_plus, float *p_minus, uint8_t *s_src_prev, uint8_t *s_tgt_prev, const uint8_t *s_src,
                                       const uint8_t *s_tgt, int B, int Nin, int N, float reward, const float *reward_vec, float nu0,
                                       float a_plus, float a_minus, float decay_plus, float decay_minus, float wdecay, int has_min, float wmin,
                                       int has_max, float wmax, int squeeze, float *ring, int K, int continuous, int idx, int reduce) {
    if (K < 1 || K > kAvgMaxTerms || idx < 0 || idx >= K) return -1;
    AvgMstdp a;
    a.p_plus = p_plus; a.p_minus = p_minus; a.s_src_prev = s_src_prev; a.s_tgt_prev = s_tgt_prev;
    a.B = B; a.Nin = Nin; a.N = N;
    a.reward = reward; a.reward_vec = reward_vec; a.nu0 = nu0; a.squeeze = squeeze;
    a.fin = AvgBounds{wdecay, has_min, wmin, has_max, wmax};
    a.ring = avg_ring(ring, K, idx, continuous);
    DISPATCH(avg_mstdp_all, W, a)
    for (long k = 0; k < (long)B * ((long)Nin + N); ++k)
        avg_trace_elem(p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, (long)B * Nin, k, a_plus, a_minus, decay_plus, decay_minus);
    return 0;
}

// ---- PostPre on a float16 / bfloat16 Weight: masks packed as k_postpre_h16 packs them ----------------------------------------------
template <int DT, int R>
static void half_all(uint16_t *W, const HalfPostPre &a) {
    const int MW = (a.B + 31) / 32;
    std::vector<uint32_t> mS((size_t)a.Nin * MW, 0u), mT((size_t)a.N * MW, 0u);
    for (int b = 0; b < a.B; ++b) {
        for (int i = 0; i < a.Nin; ++i) if (a.s_src[(size_t)b * a.Nin + i]) mS[(size_t)i * MW + (b >> 5)] |= 1u << (b & 31);
        for (int j = 0; j < a.N; ++j) if (a.s_tgt[(size_t)b * a.N + j]) mT[(size_t)j * MW + (b >> 5)] |= 1u << (b & 31);
    }
    for (int i = 0; i < a.Nin; ++i)
        for (int j = 0; j < a.N; ++j) {
            const size_t e = (size_t)i * a.N + j;
            W[e] = half_postpre_elem<DT, R>(W[e], a, i, j, &mS[(size_t)i * MW], 1, &mT[(size_t)j * MW], 1);
        }
}
template <int R>
static void half_both(uint16_t *W, int w_dtype, const HalfPostPre &a) {
    if (w_dtype == kWF16) half_all<kWF16, R>(W, a); else half_all<kWBF16, R>(W, a);
}

extern "C" int hostcheck_half_postpre_red(uint16_t *W, int w_dtype, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                                          const float *x_tgt, int B, int Nin, int N, float nu0, float nu1, int use_dt, float dt, float decay,
                                          int has_min, float wmin, int has_max, float wmax, int reduce) {
    if ((w_dtype != kWF16 && w_dtype != kWBF16) || B > kHalfMaxB) return -1;
    const HalfPostPre a{s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, use_dt, dt, decay, has_min, wmin, has_max, wmax};
    DISPATCH(half_both, W, w_dtype, a)
    return 0;
}

// ---- Conv2dConnection, phase 2: k_conv_pp_apply (mode 0) / k_conv_hebb_apply (1 Hebbian, 2 WeightDependentPostPre) over part [2][B][E] ----
template <int R>
static void conv_apply_all(float *W, const float *part, int B, long E, int mode, float nu0, float nu1, float decay, int has_min, float wmin,
                           int has_max, float wmax) {
    using ACC = BatchReduce<R>;
    for (long e = 0; e < E; ++e) {
        const bool tail = e >= (E / 32) * 32;
        float w = W[e];
        if (mode == 0) {
            if (nu0 != 0.f) w = w - nu0 * conv_pp_batch_sum<ACC>(part, B, E, e, tail);
            if (nu1 != 0.f) w = w + nu1 * conv_pp_batch_sum<ACC>(part + (size_t)B * E, B, E, e, tail);
        } else {
            const int weight_dependent = mode == 2;
            const float pre = (!weight_dependent || nu0 != 0.f) ? conv_pp_batch_sum<ACC>(part, B, E, e, tail) : 0.f;
            const float post = (!weight_dependent || nu1 != 0.f) ? conv_pp_batch_sum<ACC>(part + (size_t)B * E, B, E, e, tail) : 0.f;
            if (!weight_dependent) {
                w = w + nu0 * pre;
                w = w + nu1 * post;
            } else {
                float upd = 0.f;
                if (nu0 != 0.f) upd = upd - (nu0 * pre) * (w - wmin);
                if (nu1 != 0.f) upd = upd + (nu1 * post) * (wmax - w);
                w = w + upd;
            }
        }
        w = w * decay;
        if (has_min && w < wmin) w = wmin;
        if (has_max && w > wmax) w = wmax;
        W[e] = w;
    }
}

extern "C" int hostcheck_conv_apply(float *W, const float *part, int B, long E, int mode, float nu0, float nu1, float decay, int has_min,
                                    float wmin, int has_max, float wmax, int reduce) {
    DISPATCH(conv_apply_all, W, part, B, E, mode, nu0, nu1, decay, has_min, wmin, has_max, wmax)
    return 0;
}

// ---- LocalConnection1D / 2D / 3D: k_local_postpre's statements; src int32 [Cin, conv_prod, kernel_prod], W [R = F*conv_prod, Cin*kernel_prod] ----
template <int R_>
static void local_all(float *W, const int *src, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                      int Cin, int R, int conv_prod, int kernel_prod, int n_src, float nu0, float nu1, float decay, int has_min, float wmin,
                      int has_max, float wmax) {
    const long J = (long)Cin * kernel_prod, E = (long)R * J, CK = (long)conv_prod * kernel_prod;
    for (long e = 0; e < E; ++e) {
        const int r = (int)(e / J);
        const long j = e - (long)r * J;
        const long p = (long)(r % conv_prod) * J + j;
        const int ci = (int)(p / CK);
        const long rem = p - (long)ci * CK;
        const int o = (int)(rem / kernel_prod), k = (int)(rem - (long)o * kernel_prod);
        const int si = src[((size_t)ci * conv_prod + o) * kernel_prod + k];
        const bool in = (unsigned)si < (unsigned)n_src;
        const int sc = in ? si : 0;
        float w = W[e];
        if (nu0 != 0.f) {
            const float pre = batch_sum<R_>([&](int b) {
                const float sv = in ? (float)s_src[(size_t)b * n_src + sc] : 0.0f;
                return x_tgt[(size_t)b * R + r] * sv;
            }, B, e, E);
            const float u = nu0 * pre;
            w = w - u;
        }
        if (nu1 != 0.f) {
            const float post = batch_sum<R_>([&](int b) {
                const float xv = in ? x_src[(size_t)b * n_src + sc] : 0.0f;
                return (float)s_tgt[(size_t)b * R + r] * xv;
            }, B, e, E);
            const float u = nu1 * post;
            w = w + u;
        }
        w = w * decay;
        if (has_min && w < wmin) w = wmin;
        if (has_max && w > wmax) w = wmax;
        W[e] = w;
    }
}

extern "C" int hostcheck_local_postpre(float *W, const int *src, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                                       const float *x_tgt, int B, int Cin, int R, int conv_prod, int kernel_prod, int n_src, float nu0,
                                       float nu1, float decay, int has_min, float wmin, int has_max, float wmax, int reduce) {
    DISPATCH(local_all, W, src, s_src, x_src, s_tgt, x_tgt, B, Cin, R, conv_prod, kernel_prod, n_src, nu0, nu1, decay, has_min, wmin, has_max, wmax)
    return 0;
}

// ---- Conv1dConnection / Conv3dConnection: k_convnd_postpre's statements; tab int32 [L, J], W [Cout, J] ----
template <int R>
static void convnd_all(float *W, const int *tab, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                       int Cout, int L, int J, int n_src, float nu0, float nu1, float decay, int has_min, float wmin, int has_max, float wmax) {
    const int nw = (L + 31) >> 5;
    std::vector<uint32_t> masks((size_t)B * Cout * nw);
    for (size_t k = 0; k < masks.size(); ++k) masks[k] = convnd_pack_row_word(s_tgt + (k / nw) * L, L, (int)(k % nw));
    const long E = (long)Cout * J;
    for (long e = 0; e < E; ++e) {
        const int co = (int)(e / J), j = (int)(e - (long)co * J);
        float w = W[e];
        if (nu0 != 0.f) {
            const float pre = batch_sum<R>([&](int b) {
                const uint8_t *ss = s_src + (size_t)b * n_src;
                return convnd_pp_pre(tab, L, J, j, x_tgt + ((size_t)b * Cout + co) * L, [&](int i) { return (float)ss[i]; });
            }, B, e, E);
            const float u = nu0 * pre;
            w = w - u;
        }
        if (nu1 != 0.f) {
            const float post = batch_sum<R>([&](int b) {
                const uint32_t *mk = masks.data() + ((size_t)b * Cout + co) * nw;
                const float *xs = x_src + (size_t)b * n_src;
                return convnd_pp_post(tab, L, J, j, [&](int k) { return mk[k]; }, [&](int i) { return xs[i]; });
            }, B, e, E);
            const float u = nu1 * post;
            w = w + u;
        }
        w = w * decay;
        if (has_min && w < wmin) w = wmin;
        if (has_max && w > wmax) w = wmax;
        W[e] = w;
    }
}

extern "C" int hostcheck_convnd_postpre(float *W, const int *tab, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt,
                                        const float *x_tgt, int B, int Cout, int L, int J, int n_src, float nu0, float nu1, float decay,
                                        int has_min, float wmin, int has_max, float wmax, int reduce) {
    DISPATCH(convnd_all, W, tab, s_src, x_src, s_tgt, x_tgt, B, Cout, L, J, n_src, nu0, nu1, decay, has_min, wmin, has_max, wmax)
    return 0;
}
