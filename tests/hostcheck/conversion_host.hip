// Host-side check of bindsnet_amd/csrc/snn_conversion.hip: the __host__ __device__ bodies of csrc/snn_conversion.hpp (sif_update,
// sif_summed, pass_spike, gather_src / gather_value / gather_emit, gather_valid) and trace_next of csrc/snn_common.hpp are run
// HERE on the CPU, element by element as a kernel thread runs them, and compared with torch's own expressions by
// tests/test_conversion_hostcheck.py.  Compiled by hipcc like the kernels (same front end, -ffp-contract=off); no device code is
// executed.  Test infrastructure only; not part of libsnnhip.
#include <stdint.h>
#include "../../bindsnet_amd/csrc/snn_common.hpp"
#include "../../bindsnet_amd/csrc/snn_conversion.hpp"

using namespace snn;

// k_sif's thread per element, T steps.  cur [T, n]; trace_scale_vec nullable [n] (the PV instance's row); summed nullable [n];
// raster [T, n], vrec [T, n].
extern "C" void hostcheck_sif_run(float *v, float *refrac, uint8_t *s, float *x, float *summed, const float *cur, int T, long n,
                                  const snn_lif_params *pp, const float *trace_scale_vec, uint8_t *raster, float *vrec) {
    const snn_lif_params p = *pp;
    for (int t = 0; t < T; ++t)
        for (long k = 0; k < n; ++k) {
            const float c = cur[(size_t)t * n + k];
            float vv = v[k], rc = refrac[k];
            const uint8_t sp = sif_update(vv, rc, c, p);
            v[k] = vv; refrac[k] = rc; s[k] = sp;
            if (p.traces) x[k] = trace_next(x[k], sp, p.trace_decay, trace_scale_vec ? trace_scale_vec[k] : p.trace_scale, p.traces_additive);
            if (summed) summed[k] = sif_summed(summed[k], c);
            raster[(size_t)t * n + k] = sp;
            vrec[(size_t)t * n + k] = vv;
        }
}

extern "C" void hostcheck_pass(uint8_t *s, const float *cur, long n) {
    for (long k = 0; k < n; ++k) s[k] = pass_spike(cur[k]);
}

// k_gather's thread per output element.  Returns 0, or -1 where gather_valid refuses the geometry (nothing is read then).
extern "C" int hostcheck_gather(const uint8_t *s, float *out, long B, long n_src, const int *out_ext, const int *src_ext, const int *stride,
                                const int *off, int accumulate) {
    GatherGeom g;
    long n_out = 1;
    for (int a = 0; a < 3; ++a) {
        g.out[a] = out_ext[a]; g.src[a] = src_ext[a]; g.stride[a] = stride[a]; g.off[a] = off[a];
        n_out *= out_ext[a];
    }
    if (!gather_valid(g, n_src, n_out)) return -1;
    for (long k = 0; k < B * n_out; ++k) {
        const long b = k / n_out, j = k - b * n_out;
        const long i = gather_src(g, j);
        if (i >= n_src) return -2;                               // (cannot happen behind gather_valid: the test's own bound)
        out[k] = gather_emit(gather_value(s + b * n_src, g, j), accumulate ? out[k] : 0.0f, accumulate);
    }
    return 0;
}
