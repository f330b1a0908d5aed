// snn_run.hip -- Network.run() in C++: the per-timestep scheduler of
// bindsnet/network/network.py:380-465 driving the gfx950 kernels.
//
// Plan "generic": per-operator launches in exactly the reference's order (connections in
// insertion order feed `zeros + c1 + c2`, layers step in insertion order, then learning rules,
// monitors are written by the node kernels themselves, normalisation after the loop).
// Fused plans (below) replace the whole step by one launch for graphs they recognise.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/snnhip.h"
#include "snn_common.hpp"
#include "snn_synparams.hpp"
#include "snn_pool.hpp"
#include "snn_conversion.hpp"
#include "snn_avgpool.hpp"

static thread_local const char *g_plan = "none";
static int g_plan_mode = 0;

// ---- profiling samples (bench.py roofline) ------------------------------------------------------
static int g_prof_stride = 0;
static constexpr int kMaxSamples = 256;
static hipEvent_t g_ev0[kMaxSamples], g_ev1[kMaxSamples];
static int g_nsamples = 0;
static bool g_ev_ready = false;

extern "C" void snn_profile_enable(int stride) { g_prof_stride = stride > 0 ? stride : 0; g_nsamples = 0; }

bool snn_prof_active() { return g_prof_stride > 0; }

bool snn_prof_begin(int t, hipStream_t st) {
    if (!g_prof_stride || t % g_prof_stride || g_nsamples >= kMaxSamples) return false;
    if (!g_ev_ready) {
        for (int i = 0; i < kMaxSamples; ++i) { (void)hipEventCreate(&g_ev0[i]); (void)hipEventCreate(&g_ev1[i]); }
        g_ev_ready = true;
    }
    (void)hipEventRecord(g_ev0[g_nsamples], st);
    return true;
}
void snn_prof_end(hipStream_t st) { (void)hipEventRecord(g_ev1[g_nsamples++], st); }

extern "C" int snn_profile_collect(double *sum_ms, int *n) {
    if (!sum_ms || !n) return SNN_ERR_INVALID;
    double acc = 0.0;
    for (int i = 0; i < g_nsamples; ++i) {
        float ms = 0.f;
        if (snn_check(hipEventElapsedTime(&ms, g_ev0[i], g_ev1[i]))) return SNN_ERR_LAUNCH;
        acc += ms;
    }
    *sum_ms = acc; *n = g_nsamples; g_nsamples = 0;
    return SNN_OK;
}

extern "C" const char *snn_plan_name(void) { return g_plan; }
void snn_set_plan_name(const char *name) { g_plan = name; }
extern "C" void snn_set_plan_mode(int mode) { g_plan_mode = mode; }

int snn_try_fused_dc2015(const snn_layer_desc *L, int nL, const snn_conn_desc *C, int nC, const snn_run_desc *R,
                         hipStream_t st, int resident, int allow_lean, int *handled, unsigned *normalized);
int snn_try_fused_twolayer(const snn_layer_desc *L, int nL, const snn_conn_desc *C, int nC, const snn_run_desc *R,
                           hipStream_t st, int *handled, unsigned *normalized);
int snn_try_fused_convlif(const snn_layer_desc *L, int nL, const snn_conn_desc *C, int nC, const snn_run_desc *R,
                          hipStream_t st, int *handled);
int snn_try_fused_convpp(const snn_layer_desc *L, int nL, const snn_conn_desc *C, int nC, const snn_run_desc *R, hipStream_t st, int *handled);

int snn_launch_dc_membrane(float *v, float *refrac, uint8_t *s, float *theta, const float *I, int B, int N,
                           const snn_dc_params &p, long long *cursor, float *raster_v, hipStream_t st, const snn_pervec *pv);
int snn_launch_dc_arbitrate(uint8_t *s, float *x, int B, int N, const snn_dc_params &p, const float *Q, long long q_len,
                            long long *cursor, int *status, uint8_t *raster_s, hipStream_t st, const snn_pervec *pv);
int snn_launch_rng_fill(snn_rng_state *rng, const uint8_t *s, int B, int N, float *qbuf, long long *cursor,
                        hipStream_t st);

bool snn_dense_prop_takes(int Nin, int asked);            // snn_mfma.hip

#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// ---- run(..., clamp / unclamp / injects_v / masks): small elementwise helpers of the generic plan (network.py:395-449)
__global__ __launch_bounds__(256) void k_clamp(uint8_t *__restrict__ s, uint8_t *__restrict__ raster, const uint8_t *__restrict__ clamp,
                                               const uint8_t *__restrict__ unclamp, long total, int n) {
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long)gridDim.x * 256) {
        const int j = (int)(k % n);
        uint8_t v = s[k];
        if (clamp && clamp[j]) v = 1;                  // :416-421
        if (unclamp && unclamp[j]) v = 0;              // :424-429
        s[k] = v;
        if (raster) raster[k] = v;                     // monitors record after the clamps
    }
}
__global__ __launch_bounds__(256) void k_inject(float *__restrict__ v, const float *__restrict__ inj, long total, int len) {
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long)gridDim.x * 256) v[k] = v[k] + inj[k % len];   // :399-404
}
__global__ __launch_bounds__(256) void k_add_current(float *__restrict__ cur, const float *__restrict__ ext, long total) {
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long)gridDim.x * 256) cur[k] = cur[k] + ext[k];      // network.py:386-392
}
__global__ __launch_bounds__(256) void k_mask_fill(float *__restrict__ W, const uint8_t *__restrict__ mask, long total) {
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long)gridDim.x * 256) if (mask[k]) W[k] = 0.f;     // topology.py:129-133
}
// MulticompartmentConnection(traces=True): the connection's activity [B, N] feeds the target's current -- the first contribution
// is stored, a later one added as the accumulate path of the propagation kernels adds its own sum (`*dst + acc`)
__global__ __launch_bounds__(256) void k_feed_activity(float *__restrict__ cur, const float *__restrict__ act, long total, int accumulate) {
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long)gridDim.x * 256) cur[k] = accumulate ? cur[k] + act[k] : act[k];
}
static unsigned grid_for(long n) { const long g = (n + 255) / 256; return (unsigned)(g < 4096 ? (g > 0 ? g : 1) : 4096); }

// The per-neuron vectors of a layer as its step reads them: d.pv, with thresh_vec (the older field) standing in for the threshold
// where d.pv names none.
static snn_pervec layer_pervec(const snn_layer_desc &d) {
    snn_pervec pv = d.pv;
    if (!pv.v[SNN_PV_THRESH]) pv.v[SNN_PV_THRESH] = d.thresh_vec;
    return pv;
}
static bool has_pervec(const snn_layer_desc &d) {
    if (d.thresh_vec) return true;
    for (int q = 0; q < SNN_PV_COUNT; ++q) if (d.pv.v[q]) return true;
    return false;
}

static int validate_layer(const snn_layer_desc &d, const snn_run_desc *R) {
    if (d.n <= 0) return SNN_ERR_INVALID;
    if (has_pervec(d)) {       // a vector the layer's kind does not read (theta_plus on an LIF layer, say): refused up front
        unsigned allowed = 0;
        switch (d.kind) {
            case SNN_LAYER_INPUT: allowed = snn::kPvTrace; break;
            case SNN_LAYER_LIF: case SNN_LAYER_BOOSTED: allowed = snn::kPvTrace | snn::kPvThresh | snn::kPvDecay; break;
            case SNN_LAYER_DC: allowed = snn::kPvTrace | snn::kPvThresh | snn::kPvDecay | snn::kPvTheta; break;
            case SNN_LAYER_MCP: case SNN_LAYER_IF: case SNN_LAYER_IZH: allowed = snn::kPvTrace | snn::kPvThresh; break;
            case SNN_LAYER_CURRENT: allowed = snn::kPvTrace | snn::kPvThresh | snn::kPvDecay | snn::kPvIDecay; break;
            case SNN_LAYER_SRM0: allowed = snn::kPvTrace | snn::kPvThresh | snn::kPvDecay; break;
            case SNN_LAYER_CSRM: allowed = snn::kPvTrace | snn::kPvThresh | snn::kPvDecay | snn::kPvTheta; break;
            case SNN_LAYER_SIF: allowed = snn::kPvTrace; break;      // (conversion/nodes.py:93: `v[s] - thresh` takes a scalar threshold)
            case SNN_LAYER_PASS: allowed = 0; break;
            default: return SNN_ERR_INVALID;
        }
        const snn_pervec pv = layer_pervec(d);
        if (!snn::pervec_within(&pv, allowed)) return SNN_ERR_INVALID;
        if ((pv.v[SNN_PV_TRACE_DECAY] || pv.v[SNN_PV_TRACE_SCALE]) && !d.p.lif.traces) return SNN_ERR_INVALID;
        if (pv.v[SNN_PV_TRACE_SCALE] && !d.p.lif.traces_additive) return SNN_ERR_INVALID;   // (masked_fill_ takes a 0-dim value)
        // (the per-neuron instances put the sample into the grid's second dimension; an LIF layer with thresh_vec alone keeps snn_lif_step_vth)
        if (R->B > 65535 && d.kind != SNN_LAYER_SRM0 && d.kind != SNN_LAYER_CSRM && !(d.kind == SNN_LAYER_LIF && !snn::pervec_any(&d.pv))) return SNN_ERR_UNSUPPORTED;
    }
    if (d.summed && d.kind != SNN_LAYER_SIF) return SNN_ERR_INVALID;       // sum_input: SubtractiveResetIFNodes only
    if (d.kind != SNN_LAYER_INPUT && (d.ext_real || d.s_real || d.raster_real)) return SNN_ERR_INVALID;
    switch (d.kind) {
        case SNN_LAYER_PASS:              // conversion/nodes.py:122: s = x, nothing else; x must be 0 or 1 (checked per connection below)
            if (!d.s || !d.current) return SNN_ERR_INVALID;
            if (d.inject_v || d.ext_current) return SNN_ERR_UNSUPPORTED;
            break;
        case SNN_LAYER_SIF:               // conversion/nodes.py:8
            if (!d.v || !d.refrac || !d.s || !d.current) return SNN_ERR_INVALID;
            if (d.p.lif.traces && !d.x) return SNN_ERR_INVALID;
            break;
        case SNN_LAYER_INPUT:
            if (d.ext_real) {                  // a real-valued Input (snnhip.h f17): the float twins stand for ext_spikes / s / raster_s
                if (!d.s_real || d.ext_spikes || d.s || d.raster_s) return SNN_ERR_INVALID;
                if (R->B > 65535) return SNN_ERR_UNSUPPORTED;
            } else if (!d.ext_spikes || !d.s || d.s_real || d.raster_real) return SNN_ERR_INVALID;
            if (d.p.lif.traces && !d.x) return SNN_ERR_INVALID;
            break;
        case SNN_LAYER_DC:
            if (!d.theta) return SNN_ERR_INVALID;
            if (d.p.one_spike && (!R->cursor || !R->status)) return SNN_ERR_INVALID;
            if (d.p.one_spike && !R->noise_q && !(R->rng && R->qbuf)) return SNN_ERR_INVALID;
            if (R->B > 1024) return SNN_ERR_UNSUPPORTED;
            /* fallthrough */
        case SNN_LAYER_LIF:
            if (!d.v || !d.refrac || !d.s || !d.current) return SNN_ERR_INVALID;
            if (d.p.lif.traces && !d.x) return SNN_ERR_INVALID;
            break;
        case SNN_LAYER_IZH:               // nodes.py:1147: u in aux, a .. d and the transposed lateral matrix
            if (!d.aux || !d.izh_a || !d.izh_b || !d.izh_c || !d.izh_d || !d.izh_St) return SNN_ERR_INVALID;
            if (d.n > SNN_IZH_MAX_N) return SNN_ERR_UNSUPPORTED;
            if (!d.v || !d.s || !d.current) return SNN_ERR_INVALID;
            if (d.p.lif.traces && !d.x) return SNN_ERR_INVALID;
            break;
        case SNN_LAYER_SRM0:              // nodes.py:1555: draws from the run's generator; s_prob and rho are outputs
            if (!R->rng || !d.srm_sprob || !d.srm_rho || !d.refrac) return SNN_ERR_INVALID;
            if (!d.v || !d.s || !d.current) return SNN_ERR_INVALID;
            if (d.p.lif.traces && !d.x) return SNN_ERR_INVALID;
            break;
        case SNN_LAYER_CSRM:              // nodes.py:1319: a window of currents in, its own last spikes; no reset, no refractory counter
            if (!d.csrm_xwin || !d.csrm_last || !d.csrm_resk || !d.csrm_refk || !d.theta || d.csrm_wres <= 0 || d.csrm_wref <= 0) return SNN_ERR_INVALID;
            if (!d.v || !d.s) return SNN_ERR_INVALID;
            if (d.p.lif.traces && !d.x) return SNN_ERR_INVALID;
            if (d.ext_current) return SNN_ERR_UNSUPPORTED;
            if (d.csrm_wres > SNN_CSRM_MAX_WINDOW || d.csrm_wref > SNN_CSRM_MAX_WINDOW || R->B > 65535) return SNN_ERR_UNSUPPORTED;
            if ((long long)R->B * d.csrm_wres * d.n > 2147483647LL || (long long)R->B * d.csrm_wref * d.n > 2147483647LL) return SNN_ERR_UNSUPPORTED;
            break;
        case SNN_LAYER_CURRENT:           // nodes.py:681: the synaptic current i in aux
            if (!d.aux) return SNN_ERR_INVALID;
            /* fallthrough */
        case SNN_LAYER_IF:                // nodes.py:308
        case SNN_LAYER_BOOSTED:           // nodes.py:562
            if (!d.refrac) return SNN_ERR_INVALID;
            /* fallthrough */
        case SNN_LAYER_MCP:               // nodes.py:231
            if (!d.v || !d.s || !d.current) return SNN_ERR_INVALID;
            if (d.p.lif.traces && !d.x) return SNN_ERR_INVALID;
            break;
        default: return SNN_ERR_INVALID;
    }
    return SNN_OK;
}

static int validate_conn(const snn_layer_desc *L, int nL, const snn_conn_desc &d, const snn_run_desc *R) {
    if (d.src < 0 || d.src >= nL || d.dst < 0 || d.dst >= nL) return SNN_ERR_INVALID;
    if (d.activity && d.kind != SNN_CONN_MCC) return SNN_ERR_INVALID;      // traces=True: MulticompartmentConnection only (topology.py:415-435)
    if (d.pipe_n != 0) {                   // MCC with a feature pipeline: `w` only where a Weight carries the rule / the norm
        if (d.kind != SNN_CONN_MCC || d.pipe_n < 0 || d.pipe_n > SNN_MCC_MAX_PIPE || d.mask || d.bias) return SNN_ERR_INVALID;
        for (int k = 0; k < d.pipe_n; ++k) {
            if (d.pipe_kind[k] < SNN_MCC_OP_MUL_DRAW || d.pipe_kind[k] > SNN_MCC_OP_ADD_F32 || !d.pipe_val[k]) return SNN_ERR_INVALID;
            if (d.pipe_kind[k] == SNN_MCC_OP_MUL_DRAW && (!d.pipe_bits[k] || !R->rng)) return SNN_ERR_INVALID;
        }
        if (!d.w && (d.rule != SNN_RULE_NONE || d.has_norm || d.raster_w)) return SNN_ERR_INVALID;
    } else if (!d.w && d.kind != SNN_CONN_SPARSE && d.kind != SNN_CONN_POOL && d.kind != SNN_CONN_PERMUTE && d.kind != SNN_CONN_PAD && d.kind != SNN_CONN_AVGPOOL) return SNN_ERR_INVALID;
    if (L[d.dst].kind == SNN_LAYER_INPUT) return SNN_ERR_UNSUPPORTED;
    if (L[d.src].kind == SNN_LAYER_INPUT && L[d.src].ext_real) {      // out of a real-valued Input: the two ordered products, propagation only
        if ((d.kind != SNN_CONN_DENSE && d.kind != SNN_CONN_CONV2D) || d.window || L[d.dst].kind == SNN_LAYER_CSRM || d.rule != SNN_RULE_NONE)
            return SNN_ERR_UNSUPPORTED;
    }
    if ((L[d.dst].kind == SNN_LAYER_CSRM) != (d.window != 0)) return SNN_ERR_INVALID;      // topology.py:348: compute_window, and only there
    if (d.window) {                        // network.py:232-246: only Connection has a compute_window that runs
        if (d.kind != SNN_CONN_DENSE || !d.win_ring || d.win_size != L[d.dst].csrm_wres || d.win_head < 0 || d.win_head >= d.win_size) return SNN_ERR_INVALID;
        if ((long long)R->B * d.win_size * L[d.src].n > 2147483647LL) return SNN_ERR_UNSUPPORTED;
    }
    const bool conv_mstdp = d.kind == SNN_CONN_CONV2D && d.rule == SNN_RULE_MSTDP;      // learning.py:1942-2015, batch 1
    // (the three outer-product rules share the per-sample partial sums in rule_ws: learning.py:457-497, :920-976, :1348-1380; MSTDPET's conv2d
    //  form never feeds its eligibility trace, :2654-2745 -- it cannot learn and is not offered)
    const bool conv_outer = d.rule == SNN_RULE_POSTPRE || d.rule == SNN_RULE_HEBBIAN || d.rule == SNN_RULE_WDPOSTPRE;
    if (d.kind == SNN_CONN_CONV2D && d.rule != SNN_RULE_NONE && !conv_mstdp && (!conv_outer || !d.rule_ws)) return SNN_ERR_UNSUPPORTED;
    if (d.kind == SNN_CONN_CONV2D && d.rule == SNN_RULE_WDPOSTPRE && !(d.has_min && d.has_max)) return SNN_ERR_INVALID;
    if (conv_mstdp && (!d.p_plus || !d.p_minus || !d.e_trace || d.reward_vec)) return SNN_ERR_INVALID;
    if (conv_mstdp && R->B != 1) return SNN_ERR_UNSUPPORTED;
    if (d.rule == SNN_RULE_POSTPRE && (!L[d.src].x || !L[d.dst].x)) return SNN_ERR_INVALID;
    if ((d.rule == SNN_RULE_MSTDP || d.rule == SNN_RULE_MSTDPET) && !conv_mstdp && (!d.p_plus || !d.p_minus || !d.s_src_prev || !d.s_tgt_prev)) return SNN_ERR_INVALID;
    if ((d.rule == SNN_RULE_HEBBIAN || d.rule == SNN_RULE_WDPOSTPRE) && (!L[d.src].x || !L[d.dst].x)) return SNN_ERR_INVALID;
    if (d.rule == SNN_RULE_MSTDPET && (!d.e_trace || R->B != 1)) return SNN_ERR_INVALID;
    if (d.rule < SNN_RULE_NONE || d.rule > SNN_RULE_RMAX) return SNN_ERR_INVALID;
    if (d.reduce < SNN_REDUCE_SUM || d.reduce > SNN_REDUCE_AMIN) return SNN_ERR_INVALID;      // the rule's batch reduction (snnhip.h f15)
    if (d.rule == SNN_RULE_RMAX) {         // learning.py:2858-2960: a dense matrix into an SRM0 layer, additive source traces, batch 1
        if (d.kind != SNN_CONN_DENSE) return SNN_ERR_UNSUPPORTED;
        if (L[d.dst].kind != SNN_LAYER_SRM0 || !L[d.src].x || !L[d.src].p.lif.traces_additive || !d.e_trace) return SNN_ERR_INVALID;
        if (R->B != 1) return SNN_ERR_UNSUPPORTED;
    }
    if (d.kind < SNN_CONN_MCC || d.kind > SNN_CONN_AVGPOOL) return SNN_ERR_INVALID;
    if (d.w_dtype != SNN_W_F32) {          // a float16 / bfloat16 Weight: MCC with that one feature, no rule or PostPre, nothing that reads `w` as f32
        if (d.w_dtype != SNN_W_F16 && d.w_dtype != SNN_W_BF16) return SNN_ERR_INVALID;
        if (d.kind != SNN_CONN_MCC || d.pipe_n != 0 || (d.rule != SNN_RULE_NONE && d.rule != SNN_RULE_POSTPRE) || d.raster_w || d.mask)
            return SNN_ERR_UNSUPPORTED;
        if (d.rule == SNN_RULE_POSTPRE && R->B > 256) return SNN_ERR_UNSUPPORTED;
    }
    if (snn::syn_any(&d.syn) || d.norm_vec) {      // per-synapse rates / bounds, per-target norms: DENSE and MCC, f32, the dense family's rules
        if ((d.kind != SNN_CONN_DENSE && d.kind != SNN_CONN_MCC) || d.w_dtype != SNN_W_F32) return SNN_ERR_UNSUPPORTED;
        if (snn::syn_any(&d.syn) && (d.rule == SNN_RULE_NONE || d.rule == SNN_RULE_RMAX)) return SNN_ERR_UNSUPPORTED;
        if (!snn::syn_valid(&d.syn, L[d.dst].n)) return SNN_ERR_INVALID;
        if (d.rule == SNN_RULE_POSTPRE && ((d.syn.nu0 && d.syn.nu0_rs) || (d.syn.nu1 && d.syn.nu1_rs))) return SNN_ERR_INVALID;
        if (d.norm_vec && (!d.has_norm || !d.norm_ws)) return SNN_ERR_INVALID;
    }
    if (d.avg_k != 0) {                    // average_update (snnhip.h f14): MCC, f32, the three MCC rules, scalar rates and bounds
        if (d.kind != SNN_CONN_MCC || d.w_dtype != SNN_W_F32 || snn::syn_any(&d.syn)) return SNN_ERR_UNSUPPORTED;
        if (d.rule != SNN_RULE_POSTPRE && d.rule != SNN_RULE_MSTDP && d.rule != SNN_RULE_MSTDPET) return SNN_ERR_UNSUPPORTED;
        if (d.avg_k < 0 || !d.avg_ring0 || d.avg_i0 < 0 || d.avg_i0 >= d.avg_k) return SNN_ERR_INVALID;
        if (d.rule == SNN_RULE_POSTPRE && (!d.avg_ring1 || d.avg_i1 < 0 || d.avg_i1 >= d.avg_k)) return SNN_ERR_INVALID;
        if (d.avg_squeeze && R->B != 1) return SNN_ERR_INVALID;
        if (d.avg_k > SNN_AVG_MAX_TERMS || R->B > SNN_AVG_MAX_TERMS) return SNN_ERR_UNSUPPORTED;
    }
    if (d.norm_step != 0) {                // Weight(norm_frequency="time step") (snnhip.h f16): MCC, f32, the Weight's signed column sums; 1 = the two calls, 2 = the fused launch
        if ((d.norm_step != 1 && d.norm_step != 2) || (d.norm_step == 2 && d.pipe_n != 0) || d.kind != SNN_CONN_MCC || d.w_dtype != SNN_W_F32 || !d.w || !d.has_norm || d.norm_abs || !d.norm_ws) return SNN_ERR_INVALID;
    }
    if (d.kind == SNN_CONN_PERMUTE || d.kind == SNN_CONN_PAD) {        // PermuteConnection / ConstantPad2dConnection: a gather, propagation only
        if (d.rule != SNN_RULE_NONE) return SNN_ERR_UNSUPPORTED;
        if (d.has_norm || d.mask || d.raster_w || d.bias || d.w) return SNN_ERR_INVALID;
        snn::GatherGeom g;
        for (int a = 0; a < 3; ++a) { g.out[a] = d.gat_out[a]; g.src[a] = d.gat_src[a]; g.stride[a] = d.gat_stride[a]; g.off[a] = d.gat_off[a]; }
        if (!snn::gather_valid(g, L[d.src].n, L[d.dst].n)) return SNN_ERR_INVALID;
        return SNN_OK;
    }
    if (d.kind == SNN_CONN_AVGPOOL) {      // AvgPool2dConnection: integer counts over a window, propagation only (NoOp)
        if (d.rule != SNN_RULE_NONE) return SNN_ERR_UNSUPPORTED;
        if (d.has_norm || d.mask || d.raster_w || d.bias || d.w || d.avgp_c <= 0) return SNN_ERR_INVALID;
        snn::AvgGeom g;
        if (!snn::avg_geometry(g, d.avgp_in, d.avgp_k, d.avgp_stride, d.avgp_pad, d.avgp_ceil, d.avgp_include_pad, d.avgp_divisor)) return SNN_ERR_INVALID;
        if (d.avgp_c * snn::avg_plane(g) != L[d.src].n || d.avgp_c * snn::avg_out_plane(g) != L[d.dst].n) return SNN_ERR_INVALID;
        return SNN_OK;
    }
    if (d.kind == SNN_CONN_POOL || d.kind == SNN_CONN_MEANFIELD) {     // MaxPoolNdConnection / MeanFieldConnection: propagation only (NoOp)
        if (d.rule != SNN_RULE_NONE) return SNN_ERR_UNSUPPORTED;
        if (d.has_norm || d.mask || d.raster_w || d.bias) return SNN_ERR_INVALID;
        if (d.kind == SNN_CONN_POOL) {
            if (d.w || !d.firing_rates || d.pool_c <= 0) return SNN_ERR_INVALID;
            long n_in = d.pool_c, n_out = d.pool_c;
            for (int a = 0; a < 3; ++a) {
                if (d.pool_in[a] <= 0 || d.pool_k[a] <= 0 || d.pool_stride[a] <= 0 || d.pool_pad[a] < 0 || d.pool_dil[a] <= 0) return SNN_ERR_INVALID;
                const int o = snn::pool_out_size(d.pool_in[a], d.pool_k[a], d.pool_stride[a], d.pool_pad[a], d.pool_dil[a]);
                if (o <= 0 || n_in > (1L << 31) || n_out > (1L << 31)) return SNN_ERR_INVALID;
                n_in *= d.pool_in[a];
                n_out *= o;
            }
            if (n_in != L[d.src].n || n_out != L[d.dst].n) return SNN_ERR_INVALID;
        } else {
            const long n_out = (long)R->B * L[d.dst].n;
            if (d.w_numel <= 0 || n_out % d.w_numel != 0) return SNN_ERR_INVALID;
            if ((long)R->B * L[d.src].n > (1L << 24)) return SNN_ERR_UNSUPPORTED;
        }
        return SNN_OK;
    }
    if (d.kind == SNN_CONN_SPARSE) {       // SparseConnection: propagation only (a rule densifies `w` in the reference; norm and mask raise there)
        if (d.rule != SNN_RULE_NONE || d.has_norm || d.mask || d.raster_w || d.w) return SNN_ERR_INVALID;
        if (!d.sparse_ptr || d.sparse_nnz < 0 || (d.sparse_nnz > 0 && (!d.sparse_col || !d.sparse_val))) return SNN_ERR_INVALID;
        return SNN_OK;
    }
    if (d.kind == SNN_CONN_CONVND) {       // Conv1dConnection / Conv3dConnection: no rule or PostPre (learning.py:422-455, :499-559)
        if ((d.conv_nd != 1 && d.conv_nd != 3) || d.cin <= 0 || d.conv_d <= 0 || d.h <= 0 || d.wd <= 0 || d.cout <= 0 || d.conv_kd <= 0 ||
            d.kh <= 0 || d.kw <= 0 || d.mask || d.has_norm) return SNN_ERR_INVALID;
        if ((long)d.cin * d.conv_d * d.h * d.wd != L[d.src].n) return SNN_ERR_INVALID;
        if (d.rule != SNN_RULE_NONE && d.rule != SNN_RULE_POSTPRE) return SNN_ERR_UNSUPPORTED;
        if (d.rule == SNN_RULE_POSTPRE && (!d.conv_pp_src || (long)d.cout * d.conv_pp_rows != L[d.dst].n)) return SNN_ERR_INVALID;
        return SNN_OK;
    }
    if (d.kind == SNN_CONN_LOCAL) {        // LocalConnection1D / 2D / 3D: no rule or PostPre (learning.py:208-389)
        if (!d.local_src || d.cin <= 0 || d.local_F <= 0 || d.local_conv_prod <= 0 || d.local_kernel_prod <= 0 || d.mask) return SNN_ERR_INVALID;
        if (d.local_n_src != L[d.src].n || (long)d.local_F * d.local_conv_prod != L[d.dst].n) return SNN_ERR_INVALID;
        if (d.rule != SNN_RULE_NONE && d.rule != SNN_RULE_POSTPRE) return SNN_ERR_UNSUPPORTED;
        return SNN_OK;                          // has_norm: snn_normalize_conv2d, no column scratch
    }
    if (d.has_norm && (!d.norm_ws || d.kind == SNN_CONN_CONV2D)) return SNN_ERR_INVALID;
    return SNN_OK;
}

static int validate(const snn_layer_desc *L, int nL, const snn_conn_desc *C, int nC, const snn_run_desc *R) {
    if (!L || nL <= 0 || (nC > 0 && !C) || !R || R->B <= 0 || R->T < 0) return SNN_ERR_INVALID;
    if (R->n_records < 0 || (R->n_records > 0 && !R->records)) return SNN_ERR_INVALID;      // state monitors: what snn_record_segments would refuse at t = 0, refused before anything runs
    for (int k = 0; k < R->n_records; ++k) {
        const snn_record_segment &g = R->records[k];
        if (g.bytes && (!g.src || !g.dst || (g.bytes & 3) || ((((uintptr_t)g.src) | ((uintptr_t)g.dst)) & 3))) return SNN_ERR_INVALID;
    }
    for (int l = 0; l < nL; ++l) TRY(validate_layer(L[l], R));
    for (int l = 0; l < nL; ++l) {             // a PassThroughNodes layer: exactly one feeder, and one whose outputs are 0 or 1
        if (L[l].kind != SNN_LAYER_PASS) continue;
        int feeders = 0;
        for (int c = 0; c < nC; ++c) {
            if (C[c].dst != l) continue;
            ++feeders;
            if (C[c].kind != SNN_CONN_POOL && C[c].kind != SNN_CONN_PERMUTE && C[c].kind != SNN_CONN_PAD) return SNN_ERR_UNSUPPORTED;
        }
        if (feeders != 1) return SNN_ERR_UNSUPPORTED;
    }
    for (int c = 0; c < nC; ++c) TRY(validate_conn(L, nL, C[c], R));
    return SNN_OK;
}

// spikes of layer l as seen by connections BEFORE (after=false) / AFTER (after=true) its forward() at step t
static const void *layer_spikes(const snn_layer_desc &d, int B, int t, bool after) {
    if (d.kind != SNN_LAYER_INPUT) return d.s;
    const size_t stride = (size_t)B * d.n;
    if (d.ext_real) {                          // a real-valued Input: f32 slices
        if (after) return d.ext_real + (size_t)t * stride;
        return t == 0 ? d.s_real : d.ext_real + (size_t)(t - 1) * stride;
    }
    if (after) return d.ext_spikes + (size_t)t * stride;
    return t == 0 ? d.s : d.ext_spikes + (size_t)(t - 1) * stride;
}

// normalize() of a DENSE / MCC f32 matrix: one total for every target neuron, or a per-target vector (snn_conn_desc.norm_vec)
static int normalize_conn(const snn_conn_desc &d, int Nin, int N, hipStream_t st) {
    if (d.norm_vec) return snn_normalize_pv(d.w, Nin, N, d.norm_vec, d.norm_abs, d.norm_ws, st);
    return snn_normalize(d.w, Nin, N, d.norm, d.norm_abs, d.norm_ws, st);
}

// the number of weights of a connection, as a weight monitor copies them
static size_t conn_numel(const snn_conn_desc &d, const snn_layer_desc *L) {
    if (d.kind == SNN_CONN_CONV2D) return (size_t)d.cout * d.cin * d.kh * d.kw;
    if (d.kind == SNN_CONN_LOCAL) return (size_t)d.cin * d.local_F * d.local_conv_prod * d.local_kernel_prod;
    if (d.kind == SNN_CONN_CONVND) return (size_t)d.cout * d.cin * d.conv_kd * d.kh * d.kw;
    return (size_t)L[d.src].n * L[d.dst].n;
}

// (1) one connection hands its source's spikes `sp` on to its target; `fed`: an earlier connection has written the target's currents
static int feed_conn(const snn_layer_desc *L, const snn_conn_desc &d, const snn_conn_prop *p, const snn_run_desc *R, int t, const void *spv, bool fed,
                     hipStream_t st) {
    const int B = R->B;
    const snn_layer_desc &S = L[d.src], &D = L[d.dst];
    if (S.kind == SNN_LAYER_INPUT && S.ext_real) {      // (validate_conn: DENSE or CONV2D, no window, no rule)
        const float *xr = (const float *)spv;
        if (d.kind == SNN_CONN_DENSE) return snn_prop_dense_real_f32(d.w, d.bias, xr, D.current, B, S.n, D.n, fed ? 1 : 0, st);
        return snn_prop_conv2d_real_f32(d.w, d.bias, xr, D.current, B, d.cin, d.h, d.wd, d.cout, d.kh, d.kw, d.stride, d.pad, fed ? 1 : 0, st);
    }
    const uint8_t *sp = (const uint8_t *)spv;
    // traces=True: the connection's own sum goes to its activity buffer, k_feed_activity hands it on to the target below
    const int acc = d.activity ? 0 : fed ? 1 : 0;
    float *const out = d.activity ? d.activity : D.current;
    if (d.kind == SNN_CONN_MCC && d.pipe_n > 0) {
        // one compute() of the reference: every Probability draws its [S, N] mask, in pipeline order, then the terms are summed
        snn_mcc_op ops[SNN_MCC_MAX_PIPE];
        for (int k = 0; k < d.pipe_n; ++k) {
            ops[k].kind = d.pipe_kind[k]; ops[k].scalar = d.pipe_scalar[k]; ops[k].val = d.pipe_val[k]; ops[k].bits = d.pipe_bits[k];
            if (d.pipe_kind[k] == SNN_MCC_OP_MUL_DRAW)
                TRY(snn_mcc_bernoulli(R->rng, (const float *)d.pipe_val[k], d.pipe_scalar[k], S.n, D.n, d.pipe_bits[k], st));
        }
        TRY(snn_prop_mcc_pipe_f32(ops, d.pipe_n, sp, out, B, S.n, D.n, acc, st));
        // norm_frequency="time step": the pipeline's Weight is normalised behind its compute() (topology_features.py:641-643)
        if (d.norm_step) TRY(normalize_conn(d, S.n, D.n, st));      // (validate: norm_step takes the signed sums, norm_abs == 0)
    }
    else if (d.kind == SNN_CONN_MCC && d.w_dtype != SNN_W_F32) TRY(snn_prop_cascade_h16(d.w, d.w_dtype, sp, out, B, S.n, D.n, acc, st));
    else if (d.kind == SNN_CONN_MCC && d.norm_step == 2 && d.norm_vec) TRY(snn_prop_cascade_norm_pv_f32(d.w, sp, out, B, S.n, D.n, acc, d.norm_vec, d.norm_ws, st));
    else if (d.kind == SNN_CONN_MCC && d.norm_step == 2) TRY(snn_prop_cascade_norm_f32(d.w, sp, out, B, S.n, D.n, acc, d.norm, d.norm_ws, st));
    else if (d.kind == SNN_CONN_MCC && d.norm_step) {      // ... or as the two calls: the currents from the old values, then the normalisation
        TRY(snn_prop_cascade_f32(d.w, sp, out, B, S.n, D.n, acc, st));
        TRY(normalize_conn(d, S.n, D.n, st));
    }
    else if (d.kind == SNN_CONN_MCC) TRY(snn_prop_cascade_f32(d.w, sp, out, B, S.n, D.n, acc, st));
    else if (d.window) TRY(snn_prop_window_f32(d.w, d.bias, d.win_ring, (d.win_head + t) % d.win_size, sp, D.csrm_xwin, B, d.win_size,
                                               S.n, D.n, acc, st));
    // (the body -- matrix cores or event-driven -- is chosen on the device, per tile of 16 samples: the same launches whatever the spikes are)
    else if (d.kind == SNN_CONN_DENSE && p && p->prop_auto && !p->prop_flags) return SNN_ERR_INVALID;
    else if (d.kind == SNN_CONN_DENSE && p && p->prop_flags && snn_dense_prop_takes(S.n, p->prop_auto)) {
        TRY(snn_prop_dense_auto_f32(d.w, d.bias, sp, D.current, B, S.n, D.n, acc, p->prop_flags, p->prop_counters, st));
    }
    else if (d.kind == SNN_CONN_DENSE) TRY(snn_prop_dense_f32(d.w, d.bias, sp, D.current, B, S.n, D.n, acc, st));
    else if (d.kind == SNN_CONN_SPARSE) TRY(snn_prop_sparse_f32(d.sparse_ptr, d.sparse_col, d.sparse_val, d.sparse_nnz, d.bias, sp,
                                                                D.current, B, S.n, D.n, acc, st));
    else if (d.kind == SNN_CONN_POOL) TRY(snn_prop_pool_f32(d.firing_rates, sp, D.current, B, d.pool_c, d.pool_in, d.pool_k, d.pool_stride,
                                                            d.pool_pad, d.pool_dil, d.pool_decay, acc, st));
    else if (d.kind == SNN_CONN_AVGPOOL) TRY(snn_prop_avgpool2d_f32(sp, D.current, B, d.avgp_c, d.avgp_in, d.avgp_k, d.avgp_stride, d.avgp_pad,
                                                                    d.avgp_ceil, d.avgp_include_pad, d.avgp_divisor, acc, st));
    else if (d.kind == SNN_CONN_PERMUTE || d.kind == SNN_CONN_PAD) TRY(snn_prop_gather_f32(sp, D.current, B, S.n, d.gat_out, d.gat_src, d.gat_stride,
                                                                                            d.gat_off, acc, st));
    else if (d.kind == SNN_CONN_MEANFIELD) TRY(snn_prop_meanfield_f32(d.w, d.w_numel, sp, D.current, B, S.n, D.n, acc, st));
    else if (d.kind == SNN_CONN_CONVND) TRY(snn_prop_convnd_f32(d.w, d.bias, sp, D.current, B, d.cin, d.conv_d, d.h, d.wd, d.cout,
                                                                 d.conv_kd, d.kh, d.kw, d.stride, d.pad, acc, st));
    else if (d.kind == SNN_CONN_LOCAL) TRY(snn_prop_local_f32(d.w, d.local_src, sp, D.current, B, d.cin, d.local_F,
                                                              d.local_conv_prod, d.local_kernel_prod, d.local_n_src, acc, st));
    else TRY(snn_prop_conv2d_f32(d.w, d.bias, sp, D.current, B, d.cin, d.h, d.wd, d.cout, d.kh, d.kw,
                                 d.stride, d.pad, acc, st));
    if (d.activity)
        hipLaunchKernelGGL(k_feed_activity, dim3(grid_for((long)B * D.n)), dim3(256), 0, st, D.current, d.activity, (long)B * D.n, fed ? 1 : 0);
    return SNN_OK;
}

// (2) one layer's forward() at step t; `fed`: a connection has written its currents in this step
static int step_layer(const snn_layer_desc &d, const snn_run_desc *R, int t, bool fed, hipStream_t st) {
    const int B = R->B;
    const size_t off = (size_t)t * B * d.n;
    uint8_t *rs = d.raster_s ? d.raster_s + off : nullptr;
    float *rv = d.raster_v ? d.raster_v + off : nullptr;
    const snn_pervec pvl = layer_pervec(d);
    const snn_pervec *pv = has_pervec(d) ? &pvl : nullptr;     // (NULL: every *_pv entry point is its scalar namesake)
    if (d.kind == SNN_LAYER_INPUT && d.ext_real) {          // (the monitor's copy: snn_net_run, one copy behind the plan)
        TRY(snn_input_step_real_pv(d.ext_real + off, d.p.lif.traces ? d.x : nullptr, B, d.n,
                                   d.p.lif.trace_decay, d.p.lif.trace_scale, d.p.lif.traces_additive, pv, nullptr, st));
        return SNN_OK;
    }
    if (d.kind == SNN_LAYER_INPUT) {
        TRY(snn_input_step_pv(d.ext_spikes + off, d.p.lif.traces ? d.x : nullptr, B, d.n,
                              d.p.lif.trace_decay, d.p.lif.trace_scale, d.p.lif.traces_additive, pv, rs, st));
        return SNN_OK;
    }
    if (!fed && d.kind == SNN_LAYER_CSRM) TRY(snn_check(hipMemsetAsync(d.csrm_xwin, 0, sizeof(float) * (size_t)B * d.csrm_wres * d.n, st)));
    else if (!fed) TRY(snn_check(hipMemsetAsync(d.current, 0, sizeof(float) * (size_t)B * d.n, st)));  // :409-413
    // an external current for this layer: added behind the connections' sums (:386-392).  With one_step the reference
    // OVERWRITES it for a layer that has an incoming connection: `current_inputs[l] = inputs[l][t]` is followed by
    // `current_inputs.update(self._get_inputs(layers=[l]))` (:388-393), which replaces the entry -- the current survives
    // only where no connection feeds the layer
    if (d.ext_current && !(R->one_step && fed))
        hipLaunchKernelGGL(k_add_current, dim3(grid_for((long)B * d.n)), dim3(256), 0, st, d.current, d.ext_current + off, (long)B * d.n);
    if (d.inject_v) {
        const int len = d.inject_len > 0 ? d.inject_len : d.n;
        hipLaunchKernelGGL(k_inject, dim3(grid_for((long)B * d.n)), dim3(256), 0, st, d.v,
                           d.inject_v + (d.inject_per_step ? (size_t)t * len : 0), (long)B * d.n, len);
    }
    // (an LIF layer whose only vector is thresh_vec keeps its own instance: snn_lif_step_vth)
    if (d.kind == SNN_LAYER_LIF && !snn::pervec_any(&d.pv)) TRY(snn_lif_step_vth(d.v, d.refrac, d.s, d.x, d.current, B, d.n, &d.p.lif, d.thresh_vec, rs, rv, st));
    else if (d.kind == SNN_LAYER_LIF) TRY(snn_lif_step_pv(d.v, d.refrac, d.s, d.x, d.current, B, d.n, &d.p.lif, pv, rs, rv, st));
    else if (d.kind == SNN_LAYER_MCP) TRY(snn_mcp_step_pv(d.v, d.s, d.x, d.current, B, d.n, &d.p.lif, pv, rs, rv, st));
    else if (d.kind == SNN_LAYER_IF) TRY(snn_if_step_pv(d.v, d.refrac, d.s, d.x, d.current, B, d.n, &d.p.lif, pv, rs, rv, st));
    else if (d.kind == SNN_LAYER_BOOSTED) TRY(snn_boosted_step_pv(d.v, d.refrac, d.s, d.x, d.current, B, d.n, &d.p.lif, pv, rs, rv, st));
    else if (d.kind == SNN_LAYER_CURRENT) TRY(snn_clif_step_pv(d.v, d.refrac, d.aux, d.s, d.x, d.current, B, d.n, &d.p.lif, d.aux_decay, pv, rs, rv, st));
    else if (d.kind == SNN_LAYER_IZH) TRY(snn_izh_step_pv(d.v, d.aux, d.s, d.x, d.current, d.izh_a, d.izh_b, d.izh_c, d.izh_d, d.izh_St, B, d.n,
                                                         &d.p.lif, pv, rs, rv, st));
    else if (d.kind == SNN_LAYER_SIF) TRY(snn_sif_step_pv(d.v, d.refrac, d.s, d.x, d.summed, d.current, B, d.n, &d.p.lif, pv, rs, rv, st));
    else if (d.kind == SNN_LAYER_PASS) TRY(snn_pass_step(d.s, d.current, B, d.n, rs, st));
    else if (d.kind == SNN_LAYER_CSRM) TRY(snn_csrm_step(d.v, d.s, d.x, d.theta, d.csrm_xwin, d.csrm_last, d.csrm_resk, d.csrm_wres, d.csrm_refk,
                                                        d.csrm_wref, B, d.n, &d.p, pv, rs, rv, st));
    else if (d.kind == SNN_LAYER_SRM0) TRY(snn_srm0_step_pv(R->rng, d.v, d.refrac, d.s, d.x, d.current, d.srm_sprob, d.srm_rho, B, d.n, &d.p.lif,
                                                           d.srm_eps0, d.srm_rho0, d.srm_dthresh, pv, rs, rv, st));
    else if (R->rng && d.p.one_spike) {   // device generator: membrane -> draws for this step -> arbitration
        TRY(snn_launch_dc_membrane(d.v, d.refrac, d.s, d.theta, d.current, B, d.n, d.p, R->cursor, rv, st, pv));
        TRY(snn_launch_rng_fill(R->rng, d.s, B, d.n, R->qbuf, R->cursor, st));
        TRY(snn_launch_dc_arbitrate(d.s, d.x, B, d.n, d.p, R->qbuf, (long long)B * d.n, R->cursor, R->status,
                                    rs, st, pv));
    } else TRY(snn_dc_step_pv(d.v, d.refrac, d.s, d.x, d.theta, d.current, B, d.n, &d.p, pv, R->noise_q, R->q_len,
                              R->cursor, R->status, rs, rv, st));
    // clamp / unclamp right behind the layer's own step (network.py:394-429): with one_step a later layer's
    // currents are taken from these spikes
    if (d.clamp || d.unclamp)
        hipLaunchKernelGGL(k_clamp, dim3(grid_for((long)B * d.n)), dim3(256), 0, st, d.s, rs,
                           d.clamp ? d.clamp + (d.clamp_per_step ? (size_t)t * d.n : 0) : nullptr,
                           d.unclamp ? d.unclamp + (d.unclamp_per_step ? (size_t)t * d.n : 0) : nullptr, (long)B * d.n, d.n);
    return SNN_OK;
}

// (3) one connection's learning rule at step t
static int learn_conn(const snn_layer_desc *L, const snn_conn_desc &d, const snn_run_desc *R, int t, hipStream_t st) {
    const int B = R->B;
    if (d.rule == SNN_RULE_NONE) return SNN_OK;
    const snn_layer_desc &S = L[d.src], &D = L[d.dst];
    const uint8_t *ss = (const uint8_t *)layer_spikes(S, B, t, true);      // (no rule reads a real-valued Input: validate_conn)
    if (d.rule == SNN_RULE_MSTDP && d.kind == SNN_CONN_CONV2D)
        TRY(snn_conv2d_mstdp_step(d.w, d.e_trace, d.p_plus, d.p_minus, ss, D.s, d.cin, d.h, d.wd, d.cout, d.kh, d.kw, d.stride,
                                  d.pad, d.reward, d.nu0, d.a_plus, d.a_minus, d.decay_plus, d.decay_minus, d.wdecay,
                                  d.has_min, d.wmin, d.has_max, d.wmax, st));
    else if (d.rule == SNN_RULE_POSTPRE && d.kind == SNN_CONN_LOCAL)
        TRY(snn_local_postpre_red(d.w, d.local_src, ss, S.x, D.s, D.x, B, d.cin, d.local_F, d.local_conv_prod, d.local_kernel_prod,
                                  d.local_n_src, d.nu0, d.nu1, d.wdecay, d.has_min, d.wmin, d.has_max, d.wmax, d.reduce, st));
    else if (d.rule == SNN_RULE_POSTPRE && d.kind == SNN_CONN_CONVND)
        TRY(snn_convnd_postpre_red(d.w, d.conv_pp_src, ss, S.x, D.s, D.x, B, d.cout, d.conv_pp_rows, d.cin * d.conv_kd * d.kh * d.kw,
                                   S.n, d.nu0, d.nu1, d.wdecay, d.has_min, d.wmin, d.has_max, d.wmax, (uint32_t *)d.rule_ws, d.reduce, st));
    else if (d.rule == SNN_RULE_POSTPRE && d.kind == SNN_CONN_CONV2D)
        TRY(snn_conv2d_postpre_red(d.w, ss, S.x, D.s, D.x, B, d.cin, d.h, d.wd, d.cout, d.kh, d.kw, d.stride, d.pad, d.nu0, d.nu1,
                                   d.wdecay, d.has_min, d.wmin, d.has_max, d.wmax, d.rule_ws, d.reduce, st));
    else if ((d.rule == SNN_RULE_HEBBIAN || d.rule == SNN_RULE_WDPOSTPRE) && d.kind == SNN_CONN_CONV2D)
        TRY(snn_conv2d_hebbian_red(d.w, ss, S.x, D.s, D.x, B, d.cin, d.h, d.wd, d.cout, d.kh, d.kw, d.stride, d.pad, d.nu0, d.nu1,
                                   d.rule == SNN_RULE_WDPOSTPRE, d.wdecay, d.has_min, d.wmin, d.has_max, d.wmax, d.rule_ws, d.reduce, st));
    else if (d.avg_k != 0 && d.rule == SNN_RULE_POSTPRE)           // average_update: the ring forms (snnhip.h f14); an index moves with its term
        TRY(snn_postpre_avg_step_red(d.w, ss, S.x, D.s, D.x, B, S.n, D.n, d.nu0, d.nu1, R->dt, d.wdecay, d.has_min, d.wmin, d.has_max,
                                     d.wmax, d.avg_squeeze, d.avg_ring0, d.avg_ring1, d.avg_k, d.avg_continuous,
                                     d.nu0 != 0.f ? (d.avg_i0 + t) % d.avg_k : d.avg_i0, d.nu1 != 0.f ? (d.avg_i1 + t) % d.avg_k : d.avg_i1,
                                     d.reduce, st));
    else if (d.avg_k != 0 && d.rule == SNN_RULE_MSTDP)
        TRY(snn_mstdp_avg_step_red(d.w, d.p_plus, d.p_minus, d.s_src_prev, d.s_tgt_prev, ss, D.s, B, S.n, D.n, d.reward, d.reward_vec,
                                   d.nu0, d.a_plus, d.a_minus, d.decay_plus, d.decay_minus, d.wdecay, d.has_min, d.wmin, d.has_max,
                                   d.wmax, d.avg_squeeze, d.avg_ring0, d.avg_k, d.avg_continuous, (d.avg_i0 + t) % d.avg_k, d.reduce, st));
    else if (d.avg_k != 0)
        TRY(snn_mstdpet_avg_step(d.w, d.e_trace, d.p_plus, d.p_minus, d.s_src_prev, d.s_tgt_prev, ss, D.s, S.n, D.n, d.reward,
                                 d.nu0, R->dt, d.a_plus, d.a_minus, d.decay_plus, d.decay_minus, d.decay_e, d.tc_e, d.wdecay,
                                 d.has_min, d.wmin, d.has_max, d.wmax, d.avg_ring0, d.avg_k, d.avg_continuous,
                                 (d.avg_i0 + t) % d.avg_k, st));
    else if (d.rule == SNN_RULE_POSTPRE && d.w_dtype != SNN_W_F32)
        TRY(snn_stdp_postpre_h16_red(d.w, d.w_dtype, ss, S.x, D.s, D.x, B, S.n, D.n, d.nu0, d.nu1, d.use_dt, R->dt, d.wdecay,
                                     d.has_min, d.wmin, d.has_max, d.wmax, d.reduce, st));
    else if (d.rule == SNN_RULE_RMAX)
        TRY(snn_rmax_step(d.w, d.e_trace, D.s, D.srm_sprob, S.x, S.n, D.n, d.reward, d.nu0, R->dt, d.rmax_tc_c, d.tc_e, d.wdecay,
                          d.has_min, d.wmin, d.has_max, d.wmax, st));
    // the dense family: the entry point chooses the instance from d.syn (per-synapse constants, snnhip.h f13) and d.reduce (f15)
    else if (d.rule == SNN_RULE_POSTPRE)
        TRY(snn_stdp_postpre_red(d.w, ss, S.x, D.s, D.x, B, S.n, D.n, d.nu0, d.nu1, d.use_dt, R->dt, d.wdecay,
                                 d.has_min, d.wmin, d.has_max, d.wmax, /*assume_clamped=*/t > 0 && !d.norm_step, &d.syn, d.reduce, st));
    else if (d.rule == SNN_RULE_HEBBIAN || d.rule == SNN_RULE_WDPOSTPRE)
        TRY(snn_stdp_hebbian_red(d.w, ss, S.x, D.s, D.x, B, S.n, D.n, d.nu0, d.nu1, d.rule == SNN_RULE_WDPOSTPRE, d.wdecay,
                                 d.has_min, d.wmin, d.has_max, d.wmax, &d.syn, d.reduce, st));
    else if (d.rule == SNN_RULE_MSTDP)
        TRY(snn_mstdp_step_red(d.w, d.p_plus, d.p_minus, d.s_src_prev, d.s_tgt_prev, ss, D.s, B, S.n, D.n,
                               d.reward, d.reward_vec, d.nu0, d.a_plus, d.a_minus, d.decay_plus, d.decay_minus,
                               d.wdecay, d.has_min, d.wmin, d.has_max, d.wmax, &d.syn, d.reduce, st));
    else                                   // MSTDPET (batch 1: no reduction)
        TRY(snn_mstdpet_step_pv(d.w, d.e_trace, d.p_plus, d.p_minus, d.s_src_prev, d.s_tgt_prev, ss, D.s, S.n, D.n, d.reward,
                                d.nu0, R->dt, d.a_plus, d.a_minus, d.decay_plus, d.decay_minus, d.decay_e, d.tc_e, d.wdecay,
                                d.has_min, d.wmin, d.has_max, d.wmax, &d.syn, st));
    return SNN_OK;
}

// P: the caller's snn_conn_prop table [nC] (snn_net_run_props), entry c for connection c; NULL: none
static int run_generic(const snn_layer_desc *L, int nL, const snn_conn_desc *C, int nC, const snn_conn_prop *P, const snn_run_desc *R,
                       hipStream_t st) {
    const int B = R->B;
    bool fed[64];
    if (nL > 64) return SNN_ERR_UNSUPPORTED;
    for (int t = 0; t < R->T; ++t) {
        const bool prof = snn_prof_begin(t, st);
        // (1) network.py:384 _get_inputs(): previous-step spikes through every connection, in order.  one_step
        //     (network.py:388-393): the same per target layer, right before that layer steps, from the sources' CURRENT
        //     spikes -- a source that has already stepped in this timestep (lower layer index) contributes its new ones.
        for (int l = 0; l < nL; ++l) fed[l] = false;
        auto feed = [&](int only_dst) -> int {
            for (int c = 0; c < nC; ++c) {
                const snn_conn_desc &d = C[c];
                if (only_dst >= 0 && d.dst != only_dst) continue;
                const void *sp = layer_spikes(L[d.src], B, t, only_dst >= 0 && d.src < only_dst);
                TRY(feed_conn(L, d, P ? P + c : nullptr, R, t, sp, fed[d.dst], st));
                fed[d.dst] = true;
            }
            return SNN_OK;
        };
        if (!R->one_step) TRY(feed(-1));
        // (2) network.py:386-413 layers in insertion order
        for (int l = 0; l < nL; ++l) {
            if (R->one_step && L[l].kind != SNN_LAYER_INPUT) TRY(feed(l));
            TRY(step_layer(L[l], R, t, fed[l], st));
        }
        // (3) network.py:431-454 learning rules, connection order
        if (R->learning)
            for (int c = 0; c < nC; ++c) TRY(learn_conn(L, C[c], R, t, st));
        for (int c = 0; c < nC; ++c)          // masks apply every step, learning or not (topology.py:124-133)
            if (C[c].mask && C[c].kind != SNN_CONN_CONV2D)
                hipLaunchKernelGGL(k_mask_fill, dim3(grid_for((long)L[C[c].src].n * L[C[c].dst].n)), dim3(256), 0, st, C[c].w, C[c].mask,
                                   (long)L[C[c].src].n * L[C[c].dst].n);
        for (int c = 0; c < nC; ++c)          // network.py:456-458: monitors record last, i.e. the weights this step leaves behind
            if (C[c].raster_w) {
                const size_t ne = conn_numel(C[c], L);
                if (hipMemcpyAsync(C[c].raster_w + (size_t)t * ne, C[c].w, ne * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
                    return SNN_ERR_LAUNCH;
            }
        if (R->n_records > 0) TRY(snn_record_segments(R->records, R->n_records, t, st));      // ... and the state monitors, one launch (monitors.py:94-111)
        if (prof) snn_prof_end(st);
    }
    return snn_check_launch();
}

// Spike monitors on Input layers (snn_layer_desc.raster_s of an INPUT layer): the raster of an Input layer is a copy of its input
// (monitors.py:94-111 clone `s`, which aliases the input slice), so no plan writes it step by step -- the plans see the descriptors
// WITHOUT it, and snn_net_run makes ONE device copy per monitored input behind the plan; a plan that has the copy made inside its own
// launch (third-generation D&C form: its producer workgroups, snn_dc2015_async.hip) takes the request from snn_input_raster_request()
// and says so with snn_input_raster_done().
static thread_local uint8_t *g_in_raster_req[8];
static thread_local unsigned g_in_raster_done;
uint8_t *snn_input_raster_request(int layer) { return layer >= 0 && layer < 8 ? g_in_raster_req[layer] : nullptr; }
void snn_input_raster_done(int layer) { if (layer >= 0 && layer < 8) g_in_raster_done |= 1u << layer; }

static int net_run_plans(const snn_layer_desc *L, int nL, const snn_conn_desc *C, int nC, const snn_conn_prop *P, const snn_run_desc *R, hipStream_t st);
void snn_dc2015_ws_key_in(unsigned long long key);   // snn_dc2015.hip: the caller's host_state[0] as this run found it

extern "C" int snn_net_run(const snn_layer_desc *L, int nL, const snn_conn_desc *C, int nC, const snn_run_desc *R,
                           snn_stream_t stream) {
    return snn_net_run_props(L, nL, C, nC, nullptr, R, stream);
}

// (every plan passes `C` on index for index, so entry c of P stays connection c's)
extern "C" int snn_net_run_props(const snn_layer_desc *L, int nL, const snn_conn_desc *C, int nC, const snn_conn_prop *P,
                                 const snn_run_desc *R, snn_stream_t stream) {
    TRY(validate(L, nL, C, nC, R));
    hipStream_t st = (hipStream_t)stream;
    bool any = false;
    for (int l = 0; l < nL; ++l) any = any || (L[l].kind == SNN_LAYER_INPUT && L[l].raster_s);
    for (int l = 0; l < nL; ++l)           // a real-valued Input's monitor: a copy of its f32 input, behind the run like the byte copy below
        if (L[l].kind == SNN_LAYER_INPUT && L[l].ext_real && L[l].raster_real) {
            std::vector<snn_layer_desc> Lr(L, L + nL);
            for (int k = 0; k < nL; ++k) Lr[k].raster_real = nullptr;
            TRY(snn_net_run_props(Lr.data(), nL, C, nC, P, R, stream));
            for (int k = l; k < nL; ++k)
                if (L[k].kind == SNN_LAYER_INPUT && L[k].ext_real && L[k].raster_real)
                    TRY(snn_check(hipMemcpyAsync(L[k].raster_real, L[k].ext_real, sizeof(float) * (size_t)R->T * R->B * L[k].n, hipMemcpyDeviceToDevice, (hipStream_t)stream)));
            return SNN_OK;
        }
    if (!any) return net_run_plans(L, nL, C, nC, P, R, st);
    std::vector<snn_layer_desc> L2(L, L + nL);
    g_in_raster_done = 0;
    for (int l = 0; l < nL; ++l) {
        if (l < 8) g_in_raster_req[l] = nullptr;
        if (L[l].kind != SNN_LAYER_INPUT || !L[l].raster_s) continue;
        L2[l].raster_s = nullptr;
        if (l < 8) g_in_raster_req[l] = L[l].raster_s;
    }
    const int rc = net_run_plans(L2.data(), nL, C, nC, P, R, st);
    for (int l = 0; l < nL && l < 8; ++l) g_in_raster_req[l] = nullptr;
    if (rc) return rc;
    for (int l = 0; l < nL; ++l)
        if (L[l].kind == SNN_LAYER_INPUT && L[l].raster_s && !(l < 8 && ((g_in_raster_done >> l) & 1u)))
            TRY(snn_check(hipMemcpyAsync(L[l].raster_s, L[l].ext_spikes, (size_t)R->T * R->B * L[l].n, hipMemcpyDeviceToDevice, st)));
    return SNN_OK;
}

static int net_run_plans(const snn_layer_desc *L, int nL, const snn_conn_desc *C, int nC, const snn_conn_prop *P, const snn_run_desc *R, hipStream_t st) {
    // What a pipelined caller's earlier runs knew about the workspace's content (snn_run_desc.host_state[0]: "the exchange areas are clean
    // for this layout") holds only from one chained lean D&C run to the next: EVERY run takes the word away first, and only that path puts
    // it back (snn_dc2015.hip) -- a plan that scribbles over the workspace can never leave a stale "clean" behind.
    const unsigned long long ws_key = R->host_state ? R->host_state[0] : 0ull;
    if (R->host_state) R->host_state[0] = 0ull;
    snn_dc2015_ws_key_in(ws_key);
    int handled = 0;
    unsigned normalized = 0;       // bit c: connection c was already normalised by the plan's own kernel
    int mode = g_plan_mode ? g_plan_mode : R->plan;            // the process-wide test switch wins over the per-run request
    for (int l = 0; l < nL; ++l) if (L[l].clamp || L[l].unclamp || L[l].inject_v || L[l].ext_current) mode = 1;   // only the generic plan implements these
    // (a Conv2dConnection with a rule: the generic plan, except PostPre / Hebbian / WeightDependentPostPre on the Input -> Conv2d -> LIF graph -- snn_try_fused_convpp, whole-run form only)
    bool conv_rule = false;
    for (int c = 0; c < nC; ++c) if (C[c].kind == SNN_CONN_CONV2D && C[c].rule != SNN_RULE_NONE) conv_rule = true;
    for (int c = 0; c < nC; ++c) if (C[c].mask || C[c].raster_w || C[c].activity) mode = 1;
    if (R->n_records > 0) mode = 1;                                   // state monitors: the generic plan's kernels keep x / theta / refrac_count / i in memory every step
    if (R->one_step) mode = 1;
    for (int l = 0; l < nL; ++l) if (has_pervec(L[l])) mode = 1;     // per-neuron parameters: generic plan
    bool other_nodes = false;                                          // McCullochPitts .. IzhikevichNodes, SRM0Nodes, CSRMNodes, SubtractiveResetIFNodes, PassThroughNodes: generic plan only
    for (int l = 0; l < nL; ++l) if (L[l].kind > SNN_LAYER_DC) other_nodes = true;
    bool local = false;                                                // LocalConnection1D / 2D / 3D, Conv1d / Conv3dConnection: generic
    for (int c = 0; c < nC; ++c) if (C[c].kind == SNN_CONN_LOCAL || C[c].kind == SNN_CONN_CONVND || C[c].kind >= SNN_CONN_SPARSE) local = true;   // (and SparseConnection, MaxPoolNdConnection, MeanFieldConnection, PermuteConnection, ConstantPad2dConnection) plan only; no fused plan is offered the graph
    for (int c = 0; c < nC; ++c) if (C[c].pipe_n > 0) local = true;      // an MCC feature pipeline: generic plan only as well
    for (int c = 0; c < nC; ++c) if (C[c].w_dtype != SNN_W_F32) local = true;   // ... and float16 / bfloat16 weights (the fused plans keep f32 tiles)
    for (int c = 0; c < nC; ++c) if (snn::syn_any(&C[c].syn) || C[c].norm_vec) local = true;   // ... and per-synapse rates / bounds, per-target norms
    for (int c = 0; c < nC; ++c) if (C[c].avg_k != 0) local = true;             // ... and averaged updates (the fused plans keep no ring)
    for (int c = 0; c < nC; ++c) if (C[c].norm_step != 0) local = true;         // ... and a Weight normalised every timestep (no fused plan normalises inside its loop)
    for (int c = 0; c < nC; ++c) if (C[c].reduce != SNN_REDUCE_SUM) local = true;   // ... and a batch reduction other than sum (the fused plans sum)
    for (int l = 0; l < nL; ++l) if (L[l].kind == SNN_LAYER_INPUT && L[l].ext_real) local = true;   // ... and a real-valued Input (the fused plans read spike bytes)
    if (local || other_nodes) { mode = 1; conv_rule = false; }
    if (conv_rule) {
        if (mode == 0 || mode == 3) TRY(snn_try_fused_convpp(L, nL, C, nC, R, st, &handled));
        if (!handled) mode = 1;
    }
    if (mode != 1 && !handled) TRY(snn_try_fused_dc2015(L, nL, C, nC, R, st, mode == 0 || mode == 3, mode == 0, &handled, &normalized));
    if (mode != 1 && !handled) TRY(snn_try_fused_twolayer(L, nL, C, nC, R, st, &handled, &normalized));
    if (mode != 1 && !handled) TRY(snn_try_fused_convlif(L, nL, C, nC, R, st, &handled));
    if (!handled) {
        g_plan = "generic";
        TRY(run_generic(L, nL, C, nC, P, R, st));
    }
    // network.py:464-465: normalise every connection after the loop (learning or not)
    for (int c = 0; c < nC; ++c)
        if (C[c].norm_step) continue;                         // norm_frequency="time step": connection.normalize() does nothing at the end of the run (topology_features.py:663-671)
        else if (C[c].has_norm && C[c].kind == SNN_CONN_LOCAL)     // topology.py:1601 / :1748-1759 / :1898: every [kernel_prod] row to sum `norm`
            TRY(snn_normalize_conv2d(C[c].w, C[c].cin * C[c].local_F * C[c].local_conv_prod, C[c].local_kernel_prod, C[c].norm, st));
        else if (C[c].has_norm && C[c].w_dtype != SNN_W_F32)
            TRY(snn_normalize_h16(C[c].w, C[c].w_dtype, L[C[c].src].n, L[C[c].dst].n, C[c].norm, C[c].norm_ws, st));
        else if (C[c].has_norm && (C[c].norm_vec || !((normalized >> c) & 1u)))     // (no one-launch plan takes a norm_vec)
            TRY(normalize_conn(C[c], L[C[c].src].n, L[C[c].dst].n, st));
    return SNN_OK;
}

