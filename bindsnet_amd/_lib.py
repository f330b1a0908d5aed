"""ctypes binding of libsnnhip.so (include/snnhip.h).

The library is the ONLY compute path of this package: if it is missing or a call fails, an
exception is raised -- there is no PyTorch/CPU fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsnnhip.so")
if os.environ.get("SNN_DEVELOPER") == "1" and os.environ.get("SNN_LIB_OVERRIDE"):
    # developer A/B of two builds (tools/): honoured only with SNN_DEVELOPER=1, and never silently
    import warnings
    LIB_PATH = os.environ["SNN_LIB_OVERRIDE"]
    warnings.warn(f"bindsnet_amd: SNN_LIB_OVERRIDE is active, loading {LIB_PATH} instead of the in-tree library", RuntimeWarning)

SNN_OK, SNN_ERR_NOISE, SNN_ERR_TIMEOUT, SNN_ERR_RETRY = 0, -4, -6, -7
ABI_VERSION = 8


# ---- descriptor-cache invalidation (network/network.py): every attribute assignment on a network object (layer,
# connection, feature, learning rule, monitor, the network itself) and every Module._apply (.to(), .cuda(), .float())
# advances this counter; Network.run() re-uses the descriptor arrays of its previous call only while it stands still.
_EPOCH = [0]


def epoch() -> int:
    return _EPOCH[0]


def touch() -> None:
    _EPOCH[0] += 1


class Touching:
    """Mixin: assignments to attributes of the object invalidate cached run descriptors."""

    def __setattr__(self, key, value):
        _EPOCH[0] += 1
        super().__setattr__(key, value)

    def __delattr__(self, key):
        _EPOCH[0] += 1
        super().__delattr__(key)


class TouchingModule(Touching):
    """Touching for torch.nn.Module subclasses: moving / casting the module replaces its tensors without __setattr__."""

    def _apply(self, fn, *args, **kwargs):
        _EPOCH[0] += 1
        return super()._apply(fn, *args, **kwargs)


class SnnError(RuntimeError):
    pass


def raise_if(err) -> None:           # what a `_..._refusal` piece returned: an exception, or None for "nothing against it"
    if err is not None:
        raise err


class LifParams(C.Structure):
    _fields_ = [("decay", C.c_float), ("rest", C.c_float), ("reset", C.c_float), ("thresh", C.c_float),
                ("refrac", C.c_float), ("dt", C.c_float), ("has_lbound", C.c_int), ("lbound", C.c_float),
                ("traces", C.c_int), ("trace_decay", C.c_float), ("trace_scale", C.c_float),
                ("traces_additive", C.c_int)]


class DcParams(C.Structure):
    _fields_ = [("lif", LifParams), ("theta_decay", C.c_float), ("theta_plus", C.c_float),
                ("learning", C.c_int), ("one_spike", C.c_int)]


# snn_pervec: the per-neuron quantities the step kernels read, in SNN_PV_* order (named after the layers' derived buffers)
PERVEC = ("thresh", "decay", "trace_decay", "trace_scale", "theta_decay", "theta_plus", "i_decay")


class PerVec(C.Structure):
    _fields_ = [("v", C.c_void_p * len(PERVEC))]


def pervec(vectors):
    """snn_pervec of {quantity name: f32 [n] device tensor}; None (a null pointer for the *_pv entry points) when empty."""
    if not vectors:
        return None
    pv = PerVec()
    for name, t in vectors.items():
        pv.v[PERVEC.index(name)] = t.data_ptr()
    return pv


class LayerDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("n", C.c_int), ("p", DcParams),
                ("v", C.c_void_p), ("refrac", C.c_void_p), ("x", C.c_void_p), ("theta", C.c_void_p),
                ("s", C.c_void_p), ("ext_spikes", C.c_void_p), ("raster_s", C.c_void_p),
                ("raster_v", C.c_void_p), ("current", C.c_void_p),
                ("clamp", C.c_void_p), ("unclamp", C.c_void_p), ("clamp_per_step", C.c_int), ("unclamp_per_step", C.c_int),
                ("inject_v", C.c_void_p), ("inject_per_step", C.c_int), ("inject_len", C.c_int),
                ("ext_current", C.c_void_p), ("thresh_vec", C.c_void_p),
                ("aux", C.c_void_p), ("aux_decay", C.c_float),
                ("izh_a", C.c_void_p), ("izh_b", C.c_void_p), ("izh_c", C.c_void_p), ("izh_d", C.c_void_p),
                ("izh_St", C.c_void_p), ("pv", PerVec),
                ("srm_eps0", C.c_float), ("srm_rho0", C.c_float), ("srm_dthresh", C.c_float),
                ("srm_sprob", C.c_void_p), ("srm_rho", C.c_void_p),
                ("csrm_xwin", C.c_void_p), ("csrm_last", C.c_void_p), ("csrm_resk", C.c_void_p), ("csrm_refk", C.c_void_p),
                ("csrm_wres", C.c_int), ("csrm_wref", C.c_int), ("summed", C.c_void_p),
                ("ext_real", C.c_void_p), ("s_real", C.c_void_p), ("raster_real", C.c_void_p)]


class SynParams(C.Structure):
    """snn_synparams: the per-synapse constants of a rule (include/snnhip.h f13) -- device pointers, element strides against [S, N]."""
    _fields_ = [("nu0", C.c_void_p), ("nu1", C.c_void_p), ("wmin", C.c_void_p), ("wmax", C.c_void_p),
                ("nu0_rs", C.c_int), ("nu0_cs", C.c_int), ("nu1_rs", C.c_int), ("nu1_cs", C.c_int),
                ("wmin_rs", C.c_int), ("wmin_cs", C.c_int), ("wmax_rs", C.c_int), ("wmax_cs", C.c_int),
                ("nu0_any", C.c_int), ("nu1_any", C.c_int)]


class ConnDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("src", C.c_int), ("dst", C.c_int), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("cin", C.c_int), ("h", C.c_int), ("wd", C.c_int), ("cout", C.c_int), ("kh", C.c_int),
                ("kw", C.c_int), ("stride", C.c_int), ("pad", C.c_int),
                ("rule", C.c_int), ("nu0", C.c_float), ("nu1", C.c_float), ("use_dt", C.c_int),
                ("wdecay", C.c_float), ("has_min", C.c_int), ("wmin", C.c_float), ("has_max", C.c_int),
                ("wmax", C.c_float),
                ("p_plus", C.c_void_p), ("p_minus", C.c_void_p), ("s_src_prev", C.c_void_p),
                ("s_tgt_prev", C.c_void_p), ("reward", C.c_float), ("reward_vec", C.c_void_p),
                ("a_plus", C.c_float), ("a_minus", C.c_float), ("decay_plus", C.c_float),
                ("decay_minus", C.c_float),
                ("has_norm", C.c_int), ("norm", C.c_float), ("norm_abs", C.c_int), ("norm_step", C.c_int), ("norm_ws", C.c_void_p),
                ("e_trace", C.c_void_p), ("decay_e", C.c_float), ("tc_e", C.c_float), ("rule_ws", C.c_void_p),
                ("mask", C.c_void_p), ("raster_w", C.c_void_p),
                ("local_src", C.c_void_p), ("local_F", C.c_int), ("local_conv_prod", C.c_int),
                ("local_kernel_prod", C.c_int), ("local_n_src", C.c_int),
                ("conv_nd", C.c_int), ("conv_d", C.c_int), ("conv_kd", C.c_int), ("conv_pp_src", C.c_void_p),
                ("conv_pp_rows", C.c_int),
                ("pipe_n", C.c_int), ("pipe_kind", C.c_int * 8), ("pipe_val", C.c_void_p * 8),
                ("pipe_scalar", C.c_int * 8), ("pipe_bits", C.c_void_p * 8),
                ("sparse_ptr", C.c_void_p), ("sparse_col", C.c_void_p), ("sparse_val", C.c_void_p), ("sparse_nnz", C.c_int),
                ("firing_rates", C.c_void_p), ("pool_c", C.c_int), ("pool_in", C.c_int * 3), ("pool_k", C.c_int * 3),
                ("pool_stride", C.c_int * 3), ("pool_pad", C.c_int * 3), ("pool_dil", C.c_int * 3), ("pool_decay", C.c_float),
                ("w_numel", C.c_int), ("rmax_tc_c", C.c_float),
                ("window", C.c_int), ("win_ring", C.c_void_p), ("win_head", C.c_int), ("win_size", C.c_int),
                ("gat_out", C.c_int * 3), ("gat_src", C.c_int * 3), ("gat_stride", C.c_int * 3), ("gat_off", C.c_int * 3),
                ("w_dtype", C.c_int), ("syn", SynParams), ("norm_vec", C.c_void_p),
                ("avg_ring0", C.c_void_p), ("avg_ring1", C.c_void_p), ("avg_k", C.c_int), ("avg_continuous", C.c_int),
                ("avg_squeeze", C.c_int), ("avg_i0", C.c_int), ("avg_i1", C.c_int), ("reduce", C.c_int),
                ("avgp_c", C.c_int), ("avgp_in", C.c_int * 2), ("avgp_k", C.c_int * 2), ("avgp_stride", C.c_int * 2),
                ("avgp_pad", C.c_int * 2), ("avgp_ceil", C.c_int), ("avgp_include_pad", C.c_int), ("avgp_divisor", C.c_int),
                ("activity", C.c_void_p)]


class ConnProp(C.Structure):
    """snn_conn_prop: one per connection, beside the ConnDesc array (snn_net_run_props) -- what snn_prop_dense_auto_f32 needs."""
    _fields_ = [("prop_auto", C.c_int), ("prop_flags", C.c_void_p), ("prop_counters", C.c_void_p)]


class MccOp(C.Structure):
    _fields_ = [("kind", C.c_int), ("scalar", C.c_int), ("val", C.c_void_p), ("bits", C.c_void_p)]


class RecordSegment(C.Structure):
    """snn_record_segment: timestep t copies `bytes` bytes from `src` to `dst + t * bytes` (snn_record_segments)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("bytes", C.c_ulonglong)]


class RunDesc(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("dt", C.c_float), ("learning", C.c_int),
                ("noise_q", C.c_void_p), ("q_len", C.c_longlong), ("rng", C.c_void_p), ("qbuf", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_ulonglong),
                ("cursor", C.c_void_p), ("status", C.c_void_p), ("one_step", C.c_int), ("plan", C.c_int),
                ("status2", C.c_void_p), ("host_state", C.c_void_p),
                ("records", C.POINTER(RecordSegment)), ("n_records", C.c_int)]


class FillSegment(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("bytes", C.c_ulonglong), ("pattern", C.c_uint32)]


MAX_FILL_SEGMENTS = 32
MAX_RECORD_SEGMENTS = 32  # SNN_MAX_RECORD_SEGMENTS: segments per launch of snn_record_segments (more take further launches)
LAYER_INPUT, LAYER_LIF, LAYER_DC = 0, 1, 2
LAYER_MCP, LAYER_IF, LAYER_BOOSTED, LAYER_CURRENT, LAYER_IZH, LAYER_SRM0 = 3, 4, 5, 6, 7, 8
LAYER_CSRM = 9
LAYER_SIF, LAYER_PASS = 10, 11     # bindsnet.conversion: SubtractiveResetIFNodes, PassThroughNodes
CSRM_MAX_WINDOW = 1024    # SNN_CSRM_MAX_WINDOW: the largest res_window_size / ref_window_size of a CSRMNodes layer
IZH_MAX_N = 1024          # SNN_IZH_MAX_N: the layer size up to which the lateral sum's order is pinned against torch
CONN_MCC, CONN_DENSE, CONN_CONV2D, CONN_LOCAL, CONN_CONVND, CONN_SPARSE = 0, 1, 2, 3, 4, 5
CONN_POOL, CONN_MEANFIELD = 6, 7
CONN_PERMUTE, CONN_PAD = 8, 9      # bindsnet.conversion: PermuteConnection, ConstantPad2dConnection (snn_prop_gather_f32)
CONN_AVGPOOL = 10                  # AvgPool2dConnection (snn_prop_avgpool2d_f32)
# SNN_AVGPOOL_*: windows of this many taps and more take one wave per output; the workgroup size and the largest grid of either body
AVGPOOL_COOP_TAPS, AVGPOOL_THREADS, AVGPOOL_MAX_GRID = 64, 256, 1024
POOL_STAGE = 8192        # SNN_POOL_STAGE: the largest (b, c) plane snn_prop_pool_f32 updates and pools in LDS, in one launch
MEANFIELD_STORE = 2       # SNN_MEANFIELD_STORE: snn_prop_meanfield_f32 writes mean * w itself
MEANFIELD_MAX = 1 << 24   # B * source.n up to which f32(count) / f32(numel) is the reference's mean
SPARSE_TJ = 256           # SNN_SPARSE_TJ: the column-tile width of SparseConnection's compiled form
MCC_MAX_PIPE = 8          # SNN_MCC_MAX_PIPE
MCC_OP_MUL_DRAW, MCC_OP_MUL_MASK, MCC_OP_MUL_F32, MCC_OP_ADD_F32 = 1, 2, 3, 4
AVG_MAX_TERMS = 256       # SNN_AVG_MAX_TERMS: the largest average_update (ring slots) of an MCC rule
W_F32, W_F16, W_BF16 = 0, 1, 2         # SNN_W_*: snn_conn_desc.w_dtype, the element type of a connection's `w`
REDUCE = {"sum": 0, "mean": 1, "amax": 2, "amin": 3}      # SNN_REDUCE_*: the batch reduction of a rule's update (snnhip.h f15)
RULE_NONE, RULE_POSTPRE, RULE_MSTDP, RULE_HEBBIAN, RULE_WDPOSTPRE, RULE_MSTDPET, RULE_RMAX = 0, 1, 2, 3, 4, 5, 6

_lib = None

_vp, _i, _f, _l, _ll = C.c_void_p, C.c_int, C.c_float, C.c_long, C.c_longlong
_SIGS = {
    "snn_abi_version": ([], _i),
    "snn_error_string": ([_i], C.c_char_p),
    "snn_last_hip_error": ([], C.c_char_p),
    "snn_device_count": ([], _i),
    "snn_prop_cascade_f32": ([_vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "snn_prop_mcc_pipe_f32": ([C.POINTER(MccOp), _i, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "snn_mcc_bernoulli": ([_vp, _vp, _i, _i, _i, _vp, _vp], _i),
    "snn_prop_dense_f32": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "snn_prop_sparse_f32": ([_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "snn_prop_pool_f32": ([_vp, _vp, _vp, _i, _i] + [C.POINTER(_i)] * 5 + [_f, _i, _vp], _i),
    "snn_prop_meanfield_f32": ([_vp, _i, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "snn_prop_dense_mfma_f32": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "snn_prop_dense_auto_f32": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "snn_set_dense_prop_mode": ([_i], None),
    "snn_prop_conv2d_f32": ([_vp, _vp, _vp, _vp] + [_i] * 10 + [_vp], _i),
    "snn_prop_dense_real_f32": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "snn_prop_conv2d_real_f32": ([_vp, _vp, _vp, _vp] + [_i] * 10 + [_vp], _i),
    "snn_input_step_real_pv": ([_vp, _vp, _i, _i, _f, _f, _i, C.POINTER(PerVec), _vp, _vp], _i),
    "snn_prop_local_f32": ([_vp] * 4 + [_i] * 7 + [_vp], _i),
    "snn_local_postpre": ([_vp] * 6 + [_i] * 6 + [_f] * 3 + [_i, _f, _i, _f, _vp], _i),
    "snn_prop_convnd_f32": ([_vp] * 4 + [_i] * 12 + [_vp], _i),
    "snn_convnd_postpre": ([_vp] * 6 + [_i] * 5 + [_f] * 3 + [_i, _f, _i, _f, _vp, _vp], _i),
    "snn_input_step": ([_vp, _vp, _l, _f, _f, _i, _vp, _vp], _i),
    "snn_lif_step": ([_vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), _vp, _vp, _vp], _i),
    "snn_lif_step_vth": ([_vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), _vp, _vp, _vp, _vp], _i),
    "snn_input_step_pv": ([_vp, _vp, _i, _i, _f, _f, _i, C.POINTER(PerVec), _vp, _vp], _i),
    "snn_lif_step_pv": ([_vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), C.POINTER(PerVec), _vp, _vp, _vp], _i),
    "snn_mcp_step_pv": ([_vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), C.POINTER(PerVec), _vp, _vp, _vp], _i),
    "snn_if_step_pv": ([_vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), C.POINTER(PerVec), _vp, _vp, _vp], _i),
    "snn_boosted_step_pv": ([_vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), C.POINTER(PerVec), _vp, _vp, _vp], _i),
    "snn_clif_step_pv": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), _f, C.POINTER(PerVec), _vp, _vp, _vp], _i),
    "snn_izh_step_pv": ([_vp] * 10 + [_i, _i, C.POINTER(LifParams), C.POINTER(PerVec), _vp, _vp, _vp], _i),
    "snn_dc_step_pv": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(DcParams), C.POINTER(PerVec), _vp, _ll, _vp, _vp, _vp, _vp, _vp], _i),
    "snn_srm0_step_pv": ([_vp] * 8 + [_i, _i, C.POINTER(LifParams), _f, _f, _f, C.POINTER(PerVec), _vp, _vp, _vp], _i),
    "snn_srm0_step": ([_vp] * 8 + [_i, _i, C.POINTER(LifParams), _f, _f, _f, _vp, _vp, _vp], _i),
    "snn_prop_window_f32": ([_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "snn_csrm_step": ([_vp] * 7 + [_i, _vp, _i, _i, _i, C.POINTER(DcParams), C.POINTER(PerVec), _vp, _vp, _vp], _i),
    "snn_sif_step": ([_vp] * 6 + [_i, _i, C.POINTER(LifParams), _vp, _vp, _vp], _i),
    "snn_sif_step_pv": ([_vp] * 6 + [_i, _i, C.POINTER(LifParams), C.POINTER(PerVec), _vp, _vp, _vp], _i),
    "snn_pass_step": ([_vp, _vp, _i, _i, _vp, _vp], _i),
    "snn_prop_gather_f32": ([_vp, _vp, _i, _i] + [C.POINTER(_i)] * 4 + [_i, _vp], _i),
    "snn_prop_avgpool2d_f32": ([_vp, _vp, _i, _i] + [C.POINTER(_i)] * 4 + [_i, _i, _i, _i, _vp], _i),
    "snn_set_avgpool_body": ([_i], None),
    "snn_rmax_step": ([_vp] * 5 + [_i, _i] + [_f] * 6 + [_i, _f, _i, _f, _vp], _i),
    "snn_mcp_step": ([_vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), _vp, _vp, _vp], _i),
    "snn_if_step": ([_vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), _vp, _vp, _vp], _i),
    "snn_boosted_step": ([_vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), _vp, _vp, _vp], _i),
    "snn_clif_step": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(LifParams), _f, _vp, _vp, _vp], _i),
    "snn_izh_step": ([_vp] * 10 + [_i, _i, C.POINTER(LifParams), _vp, _vp, _vp], _i),
    "snn_dc_step": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(DcParams), _vp, _ll, _vp, _vp, _vp, _vp, _vp], _i),
    "snn_dc_arbitrate": ([_vp, _vp, _i, _i, C.POINTER(DcParams), _vp, _ll, _vp, _vp, _vp, _vp], _i),
    "snn_stdp_postpre": ([_vp] * 5 + [_i, _i, _i, _f, _f, _i, _f, _f, _i, _f, _i, _f, _i, _vp], _i),
    "snn_conv2d_postpre": ([_vp] * 5 + [_i] * 9 + [_f, _f, _f, _i, _f, _i, _f, _vp, _vp], _i),
    "snn_conv2d_hebbian": ([_vp] * 5 + [_i] * 9 + [_f, _f, _i, _f, _i, _f, _i, _f, _vp, _vp], _i),
    "snn_stdp_hebbian": ([_vp] * 5 + [_i, _i, _i, _f, _f, _i, _f, _i, _f, _i, _f, _vp], _i),
    "snn_conv2d_mstdp_step": ([_vp] * 6 + [_i] * 8 + [_f] * 7 + [_i, _f, _i, _f, _vp], _i),
    "snn_mstdpet_step": ([_vp] * 8 + [_i, _i] + [_f] * 10 + [_i, _f, _i, _f, _vp], _i),
    "snn_mstdp_step": ([_vp] * 7 + [_i, _i, _i, _f, _vp, _f, _f, _f, _f, _f, _f, _i, _f, _i, _f, _vp], _i),
    "snn_normalize": ([_vp, _i, _i, _f, _i, _vp, _vp], _i),
    "snn_stdp_postpre_pv": ([_vp] * 5 + [_i, _i, _i, _f, _f, _i, _f, _f, _i, _f, _i, _f, _i, C.POINTER(SynParams), _vp], _i),
    "snn_stdp_hebbian_pv": ([_vp] * 5 + [_i, _i, _i, _f, _f, _i, _f, _i, _f, _i, _f, C.POINTER(SynParams), _vp], _i),
    "snn_mstdpet_step_pv": ([_vp] * 8 + [_i, _i] + [_f] * 10 + [_i, _f, _i, _f, C.POINTER(SynParams), _vp], _i),
    "snn_mstdp_step_pv": ([_vp] * 7 + [_i, _i, _i, _f, _vp, _f, _f, _f, _f, _f, _f, _i, _f, _i, _f, C.POINTER(SynParams), _vp], _i),
    "snn_normalize_pv": ([_vp, _i, _i, _vp, _i, _vp, _vp], _i),
    "snn_prop_cascade_norm_f32": ([_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp], _i),
    "snn_prop_cascade_norm_pv_f32": ([_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp], _i),
    "snn_postpre_avg_step": ([_vp] * 5 + [_i, _i, _i, _f, _f, _f, _f, _i, _f, _i, _f, _i, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "snn_mstdp_avg_step": ([_vp] * 7 + [_i, _i, _i, _f, _vp, _f, _f, _f, _f, _f, _f, _i, _f, _i, _f, _i, _vp, _i, _i, _i, _vp], _i),
    "snn_mstdpet_avg_step": ([_vp] * 8 + [_i, _i] + [_f] * 10 + [_i, _f, _i, _f, _vp, _i, _i, _i, _vp], _i),
    "snn_stdp_postpre_red": ([_vp] * 5 + [_i, _i, _i, _f, _f, _i, _f, _f, _i, _f, _i, _f, _i, C.POINTER(SynParams), _i, _vp], _i),
    "snn_stdp_hebbian_red": ([_vp] * 5 + [_i, _i, _i, _f, _f, _i, _f, _i, _f, _i, _f, C.POINTER(SynParams), _i, _vp], _i),
    "snn_mstdp_step_red": ([_vp] * 7 + [_i, _i, _i, _f, _vp, _f, _f, _f, _f, _f, _f, _i, _f, _i, _f, C.POINTER(SynParams), _i, _vp], _i),
    "snn_conv2d_postpre_red": ([_vp] * 5 + [_i] * 9 + [_f, _f, _f, _i, _f, _i, _f, _vp, _i, _vp], _i),
    "snn_conv2d_hebbian_red": ([_vp] * 5 + [_i] * 9 + [_f, _f, _i, _f, _i, _f, _i, _f, _vp, _i, _vp], _i),
    "snn_local_postpre_red": ([_vp] * 6 + [_i] * 6 + [_f] * 3 + [_i, _f, _i, _f, _i, _vp], _i),
    "snn_convnd_postpre_red": ([_vp] * 6 + [_i] * 5 + [_f] * 3 + [_i, _f, _i, _f, _vp, _i, _vp], _i),
    "snn_stdp_postpre_h16_red": ([_vp, _i] + [_vp] * 4 + [_i, _i, _i, _f, _f, _i, _f, _f, _i, _f, _i, _f, _i, _vp], _i),
    "snn_postpre_avg_step_red": ([_vp] * 5 + [_i, _i, _i, _f, _f, _f, _f, _i, _f, _i, _f, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "snn_mstdp_avg_step_red": ([_vp] * 7 + [_i, _i, _i, _f, _vp, _f, _f, _f, _f, _f, _f, _i, _f, _i, _f, _i, _vp, _i, _i, _i, _i, _vp], _i),
    "snn_normalize_conv2d": ([_vp, _i, _i, _f, _vp], _i),
    "snn_prop_cascade_h16": ([_vp, _i, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "snn_stdp_postpre_h16": ([_vp, _i] + [_vp] * 4 + [_i, _i, _i, _f, _f, _i, _f, _f, _i, _f, _i, _f, _vp], _i),
    "snn_normalize_h16": ([_vp, _i, _i, _i, _f, _vp, _vp], _i),
    "snn_rng_fill_exponential": ([_vp, _vp, _i, _i, _vp, _vp, _vp], _i),
    "snn_encode_bernoulli": ([_vp, _vp, _i, _i, _f, _vp, _vp], _i),
    "snn_encode_poisson": ([_vp, _i, _i, _f, C.c_ulonglong, _vp, _vp], _i),
    "snn_fill_segments": ([C.POINTER(FillSegment), _i, _vp], _i),
    "snn_record_segments": ([C.POINTER(RecordSegment), _i, _ll, _vp], _i),
    "snn_dist_unique_id": ([_vp], _i),
    "snn_dist_init": ([_i, _i, _vp, C.POINTER(_vp)], _i),
    "snn_dist_world": ([_vp, C.POINTER(_i), C.POINTER(_i)], _i),
    "snn_dist_allreduce_dw": ([_vp, _vp, _ll, _vp], _i),
    "snn_dist_allgather_step": ([_vp, _vp, _vp, _ll, _vp], _i),
    "snn_dist_destroy": ([_vp], _i),
    "snn_net_run": ([C.POINTER(LayerDesc), _i, C.POINTER(ConnDesc), _i, C.POINTER(RunDesc), _vp], _i),
    "snn_net_run_props": ([C.POINTER(LayerDesc), _i, C.POINTER(ConnDesc), _i, C.POINTER(ConnProp), C.POINTER(RunDesc), _vp], _i),
    "snn_net_workspace_bytes": ([C.POINTER(LayerDesc), _i, C.POINTER(ConnDesc), _i, C.POINTER(RunDesc)], C.c_ulonglong),
    "snn_plan_name": ([], C.c_char_p),
    "snn_dc2015_last_form": ([], C.c_int),
    "snn_set_plan_mode": ([_i], None),
    "snn_graph_stats": ([C.POINTER(C.c_int)] * 3, None),
    "snn_profile_enable": ([_i], None),
    "snn_profile_collect": ([C.POINTER(C.c_double), C.POINTER(C.c_int)], _i),
}


def exported_symbols():
    """Every symbol include/snnhip.h declares (kept in sync by tests/test_abi.py)."""
    return sorted(_SIGS)


def lib():
    """Load libsnnhip.so (built by __graft_entry__.build() / csrc/Makefile). Fails loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SnnError(f"{LIB_PATH} is missing: build it with `make -C bindsnet_amd/csrc` "
                           "(python __graft_entry__.py build). There is no fallback path.")
        L = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(L, name)          # AttributeError if the .so is stale -> loud
            fn.argtypes, fn.restype = args, res
        if L.snn_abi_version() != ABI_VERSION:
            raise SnnError(f"libsnnhip ABI {L.snn_abi_version()} != binding {ABI_VERSION}")
        _lib = L
    return _lib


def check(rc: int, what: str = ""):
    if rc != SNN_OK:
        L = lib()
        msg = L.snn_error_string(rc).decode()
        if rc == -3:
            msg += ": " + L.snn_last_hip_error().decode()
        raise SnnError(f"libsnnhip {what}: {msg} (code {rc})")


def dptr(t):
    """A tensor's address as a descriptor field (None: a null pointer)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def resident_kernel_name(form: int) -> str:
    return {3: "k_dc2015_async [lean form, third generation: compute workgroups + arbiter + raster writers + producer workgroups (the digest / X-trace "
               "pre-passes and the input monitor's copy run inside the launch)]", 2: "k_dc2015_spec [lean form, second generation]",
            1: "k_dc2015_run [lean form]"}.get(form, "k_dc2015_run")


def profile_run(net, inputs, time, stride=4, repeats=5, pipelined=False):
    """Extra run()s with HIP events around the plan's dominant launches (bench.py roofline): every `stride`-th
    timestep's launch for the per-step plans, the one launch of each run for the resident plan (`repeats` runs).
    `pipelined`: the runs are those of a Network.pipelined() section (the launch mode the caller's timed region used).
    One untimed run first: the first launch of a mode pays one-time set-up (the runtime creates the queue cooperative
    launches go through at the first of them: several ms).
    Returns {"kernel", "avg_ms", "n", "timesteps_per_launch"} or None."""
    import contextlib
    import torch
    L = lib()
    with (net.pipelined() if pipelined else contextlib.nullcontext()):
        net.run(dict(inputs), time=time)
        net.reset_state_variables()
        net.sync()
        torch.cuda.synchronize()
        L.snn_profile_enable(stride)
        try:
            for _ in range(max(1, repeats)):
                net.run(dict(inputs), time=time)
                net.reset_state_variables()
                if not net.last_plan.startswith("dc2015-resident"):
                    break
            net.sync()
            torch.cuda.synchronize()
            s, n = C.c_double(0), C.c_int(0)
            check(L.snn_profile_collect(C.byref(s), C.byref(n)), "profile_collect")
        finally:
            L.snn_profile_enable(0)
    if n.value == 0:
        return None
    plan = net.last_plan
    if plan.startswith("dc2015-resident"):
        form = L.snn_dc2015_last_form()
        return {"kernel": resident_kernel_name(form) + " (one launch per network.run())", "resident_form": form, "avg_ms": s.value / n.value, "n": n.value,
                "timesteps_per_launch": int(round(time / net.dt))}
    kernel = "k_dc2015_step (one launch per timestep)" if plan != "generic" else "generic plan: all launches of one timestep"
    return {"kernel": kernel, "avg_ms": s.value / n.value, "n": n.value, "timesteps_per_launch": 1}


def graph_stats():
    """(plain, captured, replayed) run counts of the fused plan; the last two are always 0 (no run is captured any more)."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().snn_graph_stats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value
