// half_host.hip -- the __host__ __device__ bodies of csrc/snn_half.hpp on the CPU, driven element by element as the kernels of
// csrc/snn_half.hip drive them (tests/test_half_hostcheck.py compares with torch).  Built with hipcc; no GPU is touched.
#include <stdint.h>
#include <vector>
#include "../../bindsnet_amd/csrc/snn_half.hpp"

using namespace snn;

template <int DT>
static void widen_all(const uint16_t *in, float *out, long n) { for (long k = 0; k < n; ++k) out[k] = half_widen<DT>(in[k]); }
template <int DT>
static void narrow_all(const float *in, uint16_t *out, long n) { for (long k = 0; k < n; ++k) out[k] = half_narrow<DT>(in[k]); }

// k_prop_h16: the sources of a sample in ascending order, silent ones skipped
template <int DT>
static void prop(const uint16_t *W, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate) {
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < N; ++j) {
            OuterSum acc;
            acc.init(j >= (N / 32) * 32);
            for (int i = 0; i < Nin; ++i) {
                const uint8_t sv = s[(size_t)b * Nin + i];
                if (sv) acc.add(i, half_widen<DT>(W[(size_t)i * N + j]) * (float)sv, Nin);
            }
            const size_t o = (size_t)b * N + j;
            out[o] = half_prop_finish<DT>(acc.finish(Nin), accumulate ? out[o] : 0.0f, accumulate);
        }
}

// k_postpre_h16: the spike bits of every row and column, then element by element
template <int DT>
static void postpre(uint16_t *W, const HalfPostPre &a) {
    const int MW = (a.B + 31) / 32;
    std::vector<uint32_t> mS((size_t)a.Nin * MW, 0u), mT((size_t)a.N * MW, 0u);
    for (int b = 0; b < a.B; ++b) {
        for (int i = 0; i < a.Nin; ++i) if (a.s_src[(size_t)b * a.Nin + i]) mS[(size_t)i * MW + (b >> 5)] |= 1u << (b & 31);
        for (int j = 0; j < a.N; ++j) if (a.s_tgt[(size_t)b * a.N + j]) mT[(size_t)j * MW + (b >> 5)] |= 1u << (b & 31);
    }
    for (int i = 0; i < a.Nin; ++i)
        for (int j = 0; j < a.N; ++j) {
            const size_t e = (size_t)i * a.N + j;
            W[e] = half_postpre_elem<DT>(W[e], a, i, j, &mS[(size_t)i * MW], 1, &mT[(size_t)j * MW], 1);
        }
}

template <int DT>
static void normalize(uint16_t *W, int Nin, int N, float norm, float *factor) {
    for (int j = 0; j < N; ++j) factor[j] = half_norm_factor<DT>(W, Nin, N, j, norm);
    for (long e = 0; e < (long)Nin * N; ++e) W[e] = half_norm_scale<DT>(W[e], factor[e % N]);
}

extern "C" {
int hostcheck_half_widen(const uint16_t *in, float *out, long n, int dt) {
    if (dt == kWF16) widen_all<kWF16>(in, out, n); else if (dt == kWBF16) widen_all<kWBF16>(in, out, n); else return -1;
    return 0;
}
int hostcheck_half_narrow(const float *in, uint16_t *out, long n, int dt) {
    if (dt == kWF16) narrow_all<kWF16>(in, out, n); else if (dt == kWBF16) narrow_all<kWBF16>(in, out, n); else return -1;
    return 0;
}
int hostcheck_half_prop(const uint16_t *W, int dt, const uint8_t *s, float *out, int B, int Nin, int N, int accumulate) {
    if (dt == kWF16) prop<kWF16>(W, s, out, B, Nin, N, accumulate); else if (dt == kWBF16) prop<kWBF16>(W, s, out, B, Nin, N, accumulate); else return -1;
    return 0;
}
int hostcheck_half_postpre(uint16_t *W, int dt, const uint8_t *s_src, const float *x_src, const uint8_t *s_tgt, const float *x_tgt, int B,
                           int Nin, int N, float nu0, float nu1, int use_dt, float dtv, float decay, int has_min, float wmin, int has_max,
                           float wmax) {
    if (B > kHalfMaxB) return -2;
    const HalfPostPre a{s_src, x_src, s_tgt, x_tgt, B, Nin, N, nu0, nu1, use_dt, dtv, decay, has_min, wmin, has_max, wmax};
    if (dt == kWF16) postpre<kWF16>(W, a); else if (dt == kWBF16) postpre<kWBF16>(W, a); else return -1;
    return 0;
}
int hostcheck_half_normalize(uint16_t *W, int dt, int Nin, int N, float norm, float *factor) {
    if (dt == kWF16) normalize<kWF16>(W, Nin, N, norm, factor); else if (dt == kWBF16) normalize<kWBF16>(W, Nin, N, norm, factor); else return -1;
    return 0;
}
}
