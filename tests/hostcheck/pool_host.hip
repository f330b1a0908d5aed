// Host-side check of bindsnet_amd/csrc/snn_pool.hpp: the __host__ __device__ bodies of MaxPool1d / 2d / 3dConnection.compute -- the
// rate update, the window scan with its index rule, the gather -- and of MeanFieldConnection.compute are run HERE on the CPU
// (compiled by hipcc like the kernels, no device code is executed), plane by plane as k_pool_staged / k_pool_global call them: all
// rates of a plane first, then every pooled position.  Test infrastructure only (tests/test_pool_hostcheck.py); not part of libsnnhip.
#include <stdint.h>
#include "../../bindsnet_amd/csrc/snn_pool.hpp"

static int geometry(snn::PoolGeom &g, const int *in, const int *k, const int *stride, const int *pad, const int *dil) {
    for (int a = 0; a < 3; ++a) {
        if (in[a] <= 0 || k[a] <= 0 || stride[a] <= 0 || pad[a] < 0 || dil[a] <= 0) return -1;
        g.in[a] = in[a]; g.k[a] = k[a]; g.stride[a] = stride[a]; g.pad[a] = pad[a]; g.dil[a] = dil[a];
        g.out[a] = snn::pool_out_size(in[a], k[a], stride[a], pad[a], dil[a]);
        if (g.out[a] <= 0) return -1;
    }
    return 0;
}

// one compute(): fr [planes, P] updated in place, out [planes, O] (+)= the gathered spikes
extern "C" int hostcheck_pool(float *fr, const uint8_t *s, float *out, long planes, const int *in, const int *k, const int *stride,
                              const int *pad, const int *dil, float decay, int accumulate) {
    snn::PoolGeom g;
    if (geometry(g, in, k, stride, pad, dil)) return -1;
    const long P = snn::pool_plane(g), O = snn::pool_out_plane(g);
    for (long pl = 0; pl < planes; ++pl) {
        for (long i = 0; i < P; ++i) fr[pl * P + i] = snn::pool_rate_next(fr[pl * P + i], decay, s[pl * P + i]);
        for (long o = 0; o < O; ++o) {
            float *dst = out + pl * O + o;
            *dst = snn::pool_emit(snn::pool_gather(fr + pl * P, s + pl * P, g, (int)o), accumulate ? *dst : 0.0f, accumulate);
        }
    }
    return 0;
}

// the index rule alone: idx [planes, O] for rates fr [planes, P] (any values: NaN, infinities)
extern "C" int hostcheck_pool_indices(const float *fr, long long *idx, long planes, const int *in, const int *k, const int *stride,
                                      const int *pad, const int *dil) {
    snn::PoolGeom g;
    if (geometry(g, in, k, stride, pad, dil)) return -1;
    const long P = snn::pool_plane(g), O = snn::pool_out_plane(g);
    for (long pl = 0; pl < planes; ++pl)
        for (long o = 0; o < O; ++o) {
            const int o2 = (int)(o % g.out[2]), r = (int)(o / g.out[2]);
            idx[pl * O + o] = snn::pool_argmax(fr + pl * P, g, r / g.out[1], r % g.out[1], o2);
        }
    return 0;
}

// out [n_out] (+)= mean(s [numel]) * w[o % w_numel]; mode 0: 0 + t, 1: out + t, 2: t itself
extern "C" int hostcheck_meanfield(const float *w, int w_numel, const uint8_t *s, float *out, long numel, long n_out, int mode) {
    unsigned count = 0;
    for (long i = 0; i < numel; ++i) count += s[i];
    const float mean = snn::meanfield_mean(count, (unsigned)numel);
    for (long o = 0; o < n_out; ++o) {
        const float wv = w[w_numel == 1 ? 0 : o % w_numel];
        out[o] = mode == 2 ? snn::meanfield_emit(mean, wv, 0.0f, 0) : snn::meanfield_emit(mean, wv, mode ? out[o] : 0.0f, 1);
    }
    return 0;
}
