// Host-side check of the SRM0Nodes / Rmax kernels of bindsnet_amd/csrc/snn_srm0.hip: the __host__ __device__ bodies of
// csrc/snn_common.hpp (srm0_uniform, srm0_update, rmax_constants, rmax_term, rmax_update, trace_next) and the generator helpers of
// csrc/snn_rng.hpp (mt_temper, mt_mix) are run HERE on the CPU, element by element as a kernel thread runs them, and compared with
// the reference fixtures by tests/test_srm0_hostcheck.py.  The host's expf stands in for the device's.  Compiled by hipcc like the
// kernels (same front end, -ffp-contract=off); no device code is executed.  Test infrastructure only; not part of libsnnhip.
#include <math.h>
#include <stdint.h>
#include "../../bindsnet_amd/csrc/snn_common.hpp"
#include "../../bindsnet_amd/csrc/snn_rng.hpp"

using namespace snn;

struct host_exp { float operator()(float a) const { return expf(a); } };

// k_srm0's thread per element, T steps, the draws given: cur, u [T, B*N]; thresh_vec / decay_vec nullable [N] (the PV instance).
// raster, vrec, prec (s_prob), rrec (rho): [T, B*N].
extern "C" void hostcheck_srm0_run(float *v, float *refrac, uint8_t *s, float *x, const float *cur, const float *u, int T, int B, int N,
                                   const snn_lif_params *pp, float eps_0, float rho_0, float d_thresh, const float *thresh_vec,
                                   const float *decay_vec, uint8_t *raster, float *vrec, float *prec, float *rrec) {
    const snn_lif_params p = *pp;
    const long n = (long)B * N;
    for (int t = 0; t < T; ++t)
        for (long i = 0; i < n; ++i) {
            const long j = i % N, at = (long)t * n + i;
            const float thresh = thresh_vec ? thresh_vec[j] : p.thresh, decay = decay_vec ? decay_vec[j] : p.decay;
            float vv = v[i], rc = refrac[i], pr, rh;
            const uint8_t sp = srm0_update(vv, rc, cur[at], u[at], pr, rh, p, thresh, decay, eps_0, rho_0, d_thresh, host_exp());
            v[i] = vv; refrac[i] = rc; s[i] = sp;
            if (p.traces) x[i] = trace_next(x[i], sp, p.trace_decay, p.trace_scale, p.traces_additive);
            raster[at] = sp; vrec[at] = vv; prec[at] = pr; rrec[at] = rh;
        }
}

// k_rmax's thread per synapse, T steps, from the recorded per-step target spikes s [T, N], probabilities p [T, N] and source
// traces x [T, Nin]; mask (nullable, [Nin, N]): the weights the generic plan zeroes after every step's update.
extern "C" void hostcheck_rmax_run(float *W, float *e, const uint8_t *s, const float *p, const float *x, int T, int Nin, int N, float reward,
                                   float nu0, float dt, float tc_c, float tc_e, float wdecay, int has_min, float wmin, int has_max,
                                   float wmax, const uint8_t *mask) {
    const rmax_consts c = rmax_constants(reward, nu0, dt, tc_c, tc_e);
    for (int t = 0; t < T; ++t)
        for (int j = 0; j < N; ++j) {
            const float term = rmax_term(s[(size_t)t * N + j], p[(size_t)t * N + j], c.q);
            for (int i = 0; i < Nin; ++i) {
                const size_t at = (size_t)i * N + j;
                rmax_update(W[at], e[at], term, x[(size_t)t * Nin + i], c.k, c.scale, wdecay, has_min, wmin, has_max, wmax);
                if (mask && mask[at]) W[at] = 0.f;
            }
        }
}

// The stream walk of k_srm0 on its own: `count` uniforms from the state (mt [624] raw words, *pos), which is left advanced.
extern "C" void hostcheck_stream_walk(uint32_t *mt, int *pos, long count, float *out) {
    for (long k = 0; k < count; ++k) {
        if (*pos >= 624) {
            uint32_t nx[624];
            for (int i = 0; i < 227; ++i) nx[i] = mt[i + 397] ^ mt_mix(mt[i], mt[i + 1]);
            for (int i = 227; i < 454; ++i) nx[i] = nx[i - 227] ^ mt_mix(mt[i], mt[i + 1]);
            for (int i = 454; i < 624; ++i) nx[i] = nx[i - 227] ^ mt_mix(mt[i], i == 623 ? nx[0] : mt[i + 1]);
            for (int i = 0; i < 624; ++i) mt[i] = nx[i];
            *pos = 0;
        }
        out[k] = srm0_uniform(mt_temper(mt[(*pos)++]));
    }
}
