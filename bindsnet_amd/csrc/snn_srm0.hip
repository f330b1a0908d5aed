// snn_srm0.hip -- SRM0Nodes (bindsnet/network/nodes.py:1555-1701) and its reward rule Rmax (bindsnet/learning/learning.py:2858-2960).
//
//  * snn_srm0_step: the whole step of a layer in ONE launch, draw included.  The reference draws torch.rand_like(s_prob) from the HOST
//    generator: one 32-bit mt19937 output per element, row-major over [B, N], u = (r & 0xFFFFFF) * 2^-24 -- the stream of
//    snn_encode_bernoulli and snn_mcc_bernoulli.  mt19937 has no cheap jump-ahead, so one workgroup walks the stream as
//    k_mcc_bernoulli does (the state staged in LDS, a cooperative twist per 624 words); element e of the flat range takes word e
//    of the stream and the thread that holds the word does that element's whole update (snn_common.hpp srm0_update): decay,
//    integrate, the two expf, decrement, compare, reset, clip, trace, monitor slices.  No buffer of draws, no second launch.
//    The partially consumed block goes back to *rng for whoever draws next; rng->consumed (Exp(1) draws) is not touched.
//  * snn_rmax_step: one pass over [Nin, N]; a thread keeps its column's factor s_j - p_j / (1 + (tc_c / dt) p_j) in a register
//    and walks rows, so loads and stores are coalesced along N (snn_common.hpp rmax_term / rmax_update).
// Built with -ffp-contract=off and without fast math like the other bodies: apart from the two expf (a 1-ulp function, as
// torch's own exp is) every operation is the reference's float.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_rng.hpp"

namespace {
using namespace snn;

constexpr int SNT = 256;            // 4 waves, as k_mcc_bernoulli: a 227-word twist stripe is one pass

struct dev_exp { __device__ __forceinline__ float operator()(float a) const { return expf(a); } };

// PV: the layer has per-neuron vectors (thresh, decay, trace_decay, trace_scale): neuron j = e mod N indexes them.
template <bool PV>
__global__ __launch_bounds__(SNT) void k_srm0(snn_rng_state *rng, float *__restrict__ v, float *__restrict__ refrac,
                                              uint8_t *__restrict__ s, float *__restrict__ x, const float *__restrict__ I,
                                              float *__restrict__ s_prob, float *__restrict__ rho, long long total, int N,
                                              snn_lif_params p, float eps_0, float rho_0, float d_thresh,
                                              uint8_t *__restrict__ raster_s, float *__restrict__ raster_v, snn_pervec pv) {
    __shared__ uint32_t mt[2][624];
    const int tid = threadIdx.x;
    for (int k = tid; k < 624; k += SNT) mt[0][k] = rng->mt[k];
    int pos = rng->pos, cur = 0;
    if (pos < 0 || pos > 624) pos = 624;                  // (a state image that was never filled: twist, never index past the block)
    __syncthreads();
    long long e = 0;
    while (e < total) {
        // (no barrier in front of the twist: it reads mt[cur], which the loop below only reads, and writes the buffer whose last
        //  readers passed the three barriers of the previous twist)
        if (pos >= 624) { mt_twist_block(mt[cur], mt[cur ^ 1], tid, SNT); cur ^= 1; pos = 0; }
        const int avail = (int)((long long)(624 - pos) < total - e ? (long long)(624 - pos) : total - e);
        for (int k = tid; k < avail; k += SNT) {
            const long long i = e + k;                      // < total: inside every [B, N] tensor
            const long j = PV ? (long)(i % N) : 0;
            const node_row r = row_of<PV>(p, 0.f, pv, j);
            const float u = srm0_uniform(mt_temper(mt[cur][pos + k]));
            float vv = v[i], rc = refrac[i], pr, rh;
            const uint8_t sp = srm0_update(vv, rc, I[i], u, pr, rh, p, r.thresh, r.decay, eps_0, rho_0, d_thresh, dev_exp());
            v[i] = vv; refrac[i] = rc; s[i] = sp; s_prob[i] = pr; rho[i] = rh;
            if (p.traces) x[i] = trace_next(x[i], sp, r.trace_decay, r.trace_scale, p.traces_additive);
            if (raster_s) raster_s[i] = sp;
            if (raster_v) raster_v[i] = vv;
        }
        pos += avail; e += avail;
    }
    __syncthreads();
    for (int k = tid; k < 624; k += SNT) rng->mt[k] = mt[cur][k];
    if (tid == 0) rng->pos = pos;
}

constexpr int RTX = 64, RTY = 4, RROWS = 32;      // a workgroup: 64 columns x 32 rows, 4 rows in flight

__global__ __launch_bounds__(RTX * RTY) void k_rmax(float *__restrict__ W, float *__restrict__ e_trace, const uint8_t *__restrict__ s_tgt,
                                                    const float *__restrict__ s_prob, const float *__restrict__ x_src, int Nin, int N,
                                                    float k, float q, float scale, float wdecay, int has_min, float wmin, int has_max,
                                                    float wmax) {
    const int j = blockIdx.x * RTX + threadIdx.x;
    if (j >= N) return;
    const float term = rmax_term(s_tgt[j], s_prob[j], q);
    const int i0 = blockIdx.y * RROWS, i1 = i0 + RROWS < Nin ? i0 + RROWS : Nin;
    for (int i = i0 + threadIdx.y; i < i1; i += RTY) {
        const size_t at = (size_t)i * N + j;
        float w = W[at], e = e_trace[at];
        rmax_update(w, e, term, x_src[i], k, scale, wdecay, has_min, wmin, has_max, wmax);
        W[at] = w; e_trace[at] = e;
    }
}

}  // namespace

extern "C" int snn_srm0_step_pv(snn_rng_state *rng, float *v, float *refrac, uint8_t *s, float *x, const float *I, float *s_prob,
                                float *rho, int B, int N, const snn_lif_params *h_p, float eps_0, float rho_0, float d_thresh,
                                const snn_pervec *pv, uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    if (!rng || !v || !refrac || !s || !I || !s_prob || !rho || !h_p || B <= 0 || N <= 0) return SNN_ERR_INVALID;
    if (h_p->traces && !x) return SNN_ERR_INVALID;
    const long long total = (long long)B * N;
    if (pervec_any(pv)) {
        if (!pervec_within(pv, kPvThresh | kPvDecay | kPvTrace) || (pv->v[SNN_PV_TRACE_SCALE] && !h_p->traces_additive)) return SNN_ERR_INVALID;
        hipLaunchKernelGGL(k_srm0<true>, dim3(1), dim3(SNT), 0, (hipStream_t)stream, rng, v, refrac, s, x, I, s_prob, rho, total, N, *h_p,
                           eps_0, rho_0, d_thresh, raster_s, raster_v, *pv);
    } else
        hipLaunchKernelGGL(k_srm0<false>, dim3(1), dim3(SNT), 0, (hipStream_t)stream, rng, v, refrac, s, x, I, s_prob, rho, total, N, *h_p,
                           eps_0, rho_0, d_thresh, raster_s, raster_v, snn_pervec{});
    return snn_check_launch();
}

extern "C" int snn_srm0_step(snn_rng_state *rng, float *v, float *refrac, uint8_t *s, float *x, const float *I, float *s_prob,
                             float *rho, int B, int N, const snn_lif_params *h_p, float eps_0, float rho_0, float d_thresh,
                             uint8_t *raster_s, float *raster_v, snn_stream_t stream) {
    return snn_srm0_step_pv(rng, v, refrac, s, x, I, s_prob, rho, B, N, h_p, eps_0, rho_0, d_thresh, nullptr, raster_s, raster_v, stream);
}

extern "C" int snn_rmax_step(float *W, float *e_trace, const uint8_t *s_tgt, const float *s_prob, const float *x_src, int Nin, int N,
                             float reward, float nu0, float dt, float tc_c, float tc_e, float wdecay, int has_min, float wmin,
                             int has_max, float wmax, snn_stream_t stream) {
    if (!W || !e_trace || !s_tgt || !s_prob || !x_src || Nin <= 0 || N <= 0) return SNN_ERR_INVALID;
    if ((Nin + RROWS - 1) / RROWS > 65535) return SNN_ERR_UNSUPPORTED;
    const rmax_consts c = rmax_constants(reward, nu0, dt, tc_c, tc_e);
    hipLaunchKernelGGL(k_rmax, dim3((unsigned)((N + RTX - 1) / RTX), (unsigned)((Nin + RROWS - 1) / RROWS)), dim3(RTX, RTY), 0,
                       (hipStream_t)stream, W, e_trace, s_tgt, s_prob, x_src, Nin, N, c.k, c.q, c.scale, wdecay, has_min, wmin, has_max, wmax);
    return snn_check_launch();
}
