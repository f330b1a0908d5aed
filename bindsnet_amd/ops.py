"""Thin tensor-level wrappers over the C ABI (one per entry point of include/snnhip.h).

torch is used for device memory and the current HIP stream only.  Every tensor must be a
contiguous CUDA(HIP) tensor of the documented dtype; spikes may be uint8 or bool (same byte
layout, like BindsNET's Input.s / LIFNodes.s).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import REDUCE, DcParams, LifParams, check, lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, dtype=None, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError("tensor required")
    if not t.is_cuda:
        raise _lib.SnnError("bindsnet_amd runs on an MI355X only: tensor is on " + str(t.device))
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    if dtype == "spike":
        if t.dtype not in (torch.uint8, torch.bool):
            raise TypeError(f"spike tensor must be uint8/bool, got {t.dtype}")
    elif dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


F32 = torch.float32
# Weight.value dtypes beside float32 and their snn_conn_desc.w_dtype codes: the *_h16 entry points (csrc/snn_half.hip)
HALF = {torch.float16: _lib.W_F16, torch.bfloat16: _lib.W_BF16}


def _bounds(wmin, wmax):
    """The clamp arguments of the C ABI (has_min, wmin, has_max, wmax) from optional bounds."""
    return int(wmin is not None), 0.0 if wmin is None else wmin, int(wmax is not None), 0.0 if wmax is None else wmax


def _reduce(reduce) -> int:
    """SNN_REDUCE_* of an update's `reduce` argument: "sum", "mean", "amax" or "amin" (include/snnhip.h f15)."""
    if reduce not in REDUCE:
        raise ValueError(f"reduce={reduce!r}: one of {', '.join(REDUCE)}")
    return REDUCE[reduce]


def _syn(W, nu0, nu1, wmin, wmax):
    """The rates and bounds of a dense update for the C ABI: (nu0, nu1, (has_min, wmin, has_max, wmax), snn_synparams or None,
    tensors to keep alive).  A rate or bound given as a tensor of more than one element is read per synapse by the *_pv entry
    points, broadcast against W's [Nin, N] by its strides and brought to W's device on demand."""
    from .learning._descriptor import syn_params
    nu0, nu1, lo, hi, sp, keep = syn_params(W.shape[0], W.shape[1], W.device, nu0, nu1, wmin, wmax)
    return nu0, nu1, _bounds(lo, hi), sp, keep


def prop_cascade(W, s, out, accumulate=False):
    """a5: out[b,j] (+)= sum_i W[i,j]*s[b,i] in ATen sum(dim=1) order."""
    B = s.shape[0]
    Nin, N = W.shape
    assert s.numel() == B * Nin and out.numel() == B * N
    if W.dtype in HALF:                 # a float16 / bfloat16 Weight: the f32 sum, rounded once to W's dtype, into the f32 current
        check(lib().snn_prop_cascade_h16(_ptr(W, W.dtype), HALF[W.dtype], _ptr(s, "spike"), _ptr(out, F32), B, Nin, N, int(accumulate),
                                         _stream()), "prop_cascade_h16")
        return out
    check(lib().snn_prop_cascade_f32(_ptr(W, F32), _ptr(s, "spike"), _ptr(out, F32), B, Nin, N, int(accumulate),
                                     _stream()), "prop_cascade")
    return out


def prop_cascade_norm(W, s, out, norm, accumulate=False, ws=None):
    """f16: prop_cascade(W, s, out, accumulate) from W as it was, then normalize(W, norm, use_abs=False), in one launch -- one step
    of a Weight with norm_frequency="time step".  Bit-identical to the two calls in `out` and in W; float32 only.  `norm`: a
    float, or a tensor with one total per target neuron."""
    B = s.shape[0]
    Nin, N = W.shape
    assert s.numel() == B * Nin and out.numel() == B * N
    if W.dtype != F32:
        raise NotImplementedError(f"bindsnet_amd: norm_frequency='time step' computes in float32 only (got {W.dtype})")
    if ws is None:
        ws = torch.empty(N, dtype=F32, device=W.device)
    if isinstance(norm, torch.Tensor):
        check(lib().snn_prop_cascade_norm_pv_f32(_ptr(W, F32), _ptr(s, "spike"), _ptr(out, F32), B, Nin, N, int(accumulate),
                                                 _ptr(norm_vector(norm, N, W.device), F32), _ptr(ws, F32), _stream()), "prop_cascade_norm_pv")
        return out
    check(lib().snn_prop_cascade_norm_f32(_ptr(W, F32), _ptr(s, "spike"), _ptr(out, F32), B, Nin, N, int(accumulate), float(norm),
                                          _ptr(ws, F32), _stream()), "prop_cascade_norm")
    return out


def prop_mcc_pipe(program, s, out, Nin, N, accumulate=False):
    """f8: out[b,j] (+)= sum_i term(b,i,j) of a MulticompartmentConnection feature pipeline, in ATen sum(dim=1) order.
    program: [(kind, value tensor, scalar flag, bit workspace or None)] in pipeline order (_lib.MCC_OP_*); the bit workspaces
    of the MUL_DRAW ops must have been filled by mcc_bernoulli for this call."""
    B = s.shape[0]
    assert s.numel() == B * Nin and out.numel() == B * N and 0 < len(program) <= _lib.MCC_MAX_PIPE
    arr = (_lib.MccOp * len(program))()
    for k, (kind, val, scalar, bits) in enumerate(program):
        want = torch.bool if kind == _lib.MCC_OP_MUL_MASK else F32
        if not scalar and val.numel() != Nin * N:
            raise ValueError(f"op {k}: value must have {Nin} x {N} elements")
        arr[k].kind, arr[k].scalar, arr[k].val = kind, int(bool(scalar)), _ptr(val, want)
        arr[k].bits = _ptr(bits, torch.int32) if kind == _lib.MCC_OP_MUL_DRAW else None
        if kind == _lib.MCC_OP_MUL_DRAW and bits.numel() < Nin * ((N + 31) // 32):
            raise ValueError(f"op {k}: bit workspace too small")
    check(lib().snn_prop_mcc_pipe_f32(arr, len(program), _ptr(s, "spike"), _ptr(out, F32), B, Nin, N, int(accumulate), _stream()),
          "prop_mcc_pipe")
    return out


def mcc_bernoulli(p, S, N, bits=None, rng_state=None):
    """f8: the bit-packed [S, ceil(N/32)] int32 mask torch.bernoulli(p) of an [S, N] (or one-element) f32 `p` draws.
    rng_state: the int32 image of a device generator state (rng.DeviceGenerator.state), advanced in place; None: the HOST
    generator is handed to the device for the call and left advanced by S * N outputs, as torch.bernoulli on the CPU leaves it."""
    if bits is None:
        bits = torch.empty(S * ((N + 31) // 32), dtype=torch.int32, device=p.device)
    return mcc_bernoulli_from_host([p], [bits], S, N)[0] if rng_state is None else _mcc_bernoulli(rng_state, p, S, N, bits)


def _mcc_bernoulli(rng_state, p, S, N, bits):
    if p.numel() not in (1, S * N) or bits.numel() < S * ((N + 31) // 32):
        raise ValueError(f"mcc_bernoulli: p must have 1 or {S} x {N} elements and bits {S * ((N + 31) // 32)} words")
    check(lib().snn_mcc_bernoulli(_ptr(rng_state, torch.int32), _ptr(p, F32), int(p.numel() == 1), S, N, _ptr(bits, torch.int32),
                                  _stream()), "mcc_bernoulli")
    return bits


def mcc_bernoulli_from_host(ps, bits, S, N):
    """Several consecutive draws (the Probability features of one pipeline, in order) from the HOST generator's stream: one
    hand-over to the device and back (rng.DeviceGenerator), like encode_bernoulli."""
    from .rng import DeviceGenerator
    with DeviceGenerator(ps[0].device, 1) as g:
        for p, b in zip(ps, bits):
            _mcc_bernoulli(g.state, p, S, N, b)
        g.finish()
    return bits


def prop_dense(W, s, out, bias=None, accumulate=False):
    """a6: out (+)= s @ W (+ b), ascending-i sequential f32."""
    B = s.shape[0]
    Nin, N = W.shape
    assert s.numel() == B * Nin and out.numel() == B * N
    check(lib().snn_prop_dense_f32(_ptr(W, F32), _ptr(bias, F32, True), _ptr(s, "spike"), _ptr(out, F32), B, Nin, N,
                                   int(accumulate), _stream()), "prop_dense")
    return out


def prop_dense_mfma(W, s, out, bias=None, accumulate=False):
    """a6 on the f32 matrix cores: bit-identical to prop_dense for 0/1 spikes (one k-ordered MFMA chain per tile)."""
    B = s.shape[0]
    Nin, N = W.shape
    assert s.numel() == B * Nin and out.numel() == B * N
    check(lib().snn_prop_dense_mfma_f32(_ptr(W, F32), _ptr(bias, F32, True), _ptr(s, "spike"), _ptr(out, F32), B, Nin, N,
                                        int(accumulate), _stream()), "prop_dense_mfma")
    return out


def prop_dense_auto(W, s, out, bias=None, accumulate=False, counters=None, flags=None):
    """a6 with its body chosen on the device, per tile of 16 samples: the matrix-core chain where the tile's spikes are dense and
    all 0/1, the event-driven walk elsewhere (snn_prop_dense_auto_f32).  Bit-identical to prop_dense.  `counters`: an int32 [2]
    device tensor that the call adds its {matrix, event} tile counts to; `flags`: int32 [ceil(B / 16)] scratch (made here if
    missing; afterwards 1 where the matrix body ran)."""
    B = s.shape[0]
    Nin, N = W.shape
    assert s.numel() == B * Nin and out.numel() == B * N
    tiles = (B + 15) // 16
    if flags is None:
        flags = torch.empty(tiles, dtype=torch.int32, device=W.device)
    if flags.numel() < tiles or (counters is not None and counters.numel() < 2):
        raise ValueError(f"prop_dense_auto: flags needs {tiles} int32 words, counters 2")
    check(lib().snn_prop_dense_auto_f32(_ptr(W, F32), _ptr(bias, F32, True), _ptr(s, "spike"), _ptr(out, F32), B, Nin, N,
                                        int(accumulate), _ptr(flags, torch.int32), _ptr(counters, torch.int32, True), _stream()),
          "prop_dense_auto")
    return out


def set_dense_prop_mode(mode: int) -> None:
    """Which body prop_dense_auto and the generic plan's dense connections take (tests, measurements): 0 the cost rule, 1 always
    event-driven, 2 the matrix body wherever it is exact."""
    lib().snn_set_dense_prop_mode(int(mode))


def prop_conv2d(W, s, out, bias=None, stride=1, pad=0, accumulate=False):
    """a7: F.conv2d on spikes; s [B,Cin,H,W], W [Cout,Cin,KH,KW], out [B,Cout,OH,OW]."""
    B, Cin, H, Wd = s.shape
    Cout, Cin2, KH, KW = W.shape
    assert Cin == Cin2
    check(lib().snn_prop_conv2d_f32(_ptr(W, F32), _ptr(bias, F32, True), _ptr(s, "spike"), _ptr(out, F32), B, Cin, H,
                                    Wd, Cout, KH, KW, stride, pad, int(accumulate), _stream()), "prop_conv2d")
    return out


def prop_dense_real(W, x, out, bias=None, accumulate=False):
    """f17: out (+)= x @ W (+ b) over real-valued float32 sources x [B, Nin]: ascending-i sequential f32, one rounded multiply and
    one rounded add per term, bias last (include/snnhip.h)."""
    B = x.shape[0]
    Nin, N = W.shape
    assert x.numel() == B * Nin and out.numel() == B * N
    check(lib().snn_prop_dense_real_f32(_ptr(W, F32), _ptr(bias, F32, True), _ptr(x, F32), _ptr(out, F32), B, Nin, N,
                                        int(accumulate), _stream()), "prop_dense_real")
    return out


def prop_conv2d_real(W, x, out, bias=None, stride=1, pad=0, accumulate=False):
    """f17: F.conv2d on real-valued float32 sources in the order of prop_conv2d; x [B,Cin,H,W], W [Cout,Cin,KH,KW], out [B,Cout,OH,OW]."""
    B, Cin, H, Wd = x.shape
    Cout, Cin2, KH, KW = W.shape
    assert Cin == Cin2
    check(lib().snn_prop_conv2d_real_f32(_ptr(W, F32), _ptr(bias, F32, True), _ptr(x, F32), _ptr(out, F32), B, Cin, H,
                                         Wd, Cout, KH, KW, stride, pad, int(accumulate), _stream()), "prop_conv2d_real")
    return out


def input_step_real(s, x=None, trace_decay=0.0, trace_scale=1.0, additive=False, raster=None, pv=None):
    """f17: the step of a real-valued Input layer, s float32 [B, ...]: the trace x (nullable) and the float32 raster (nullable)."""
    B = s.shape[0]
    arg, _keep = _pv(pv, s.numel() // B) if pv else (None, None)
    check(lib().snn_input_step_real_pv(_ptr(s, F32), _ptr(x, F32, True), B, s.numel() // B, trace_decay, trace_scale,
                                       int(additive), arg, _ptr(raster, F32, True), _stream()), "input_step_real")


def prop_local(W, src, s, out, n_filters, accumulate=False):
    """f5: LocalConnection1D/2D/3D.compute; W [Cin, F*conv_prod, kernel_prod] f32, src int32 [Cin, conv_prod, kernel_prod],
    s [B, n_src] spikes, out [B, F*conv_prod]."""
    B = s.shape[0]
    Cin, conv_prod, kernel_prod = src.shape
    n_src = s.numel() // B
    if tuple(W.shape) != (Cin, n_filters * conv_prod, kernel_prod) or out.numel() != B * n_filters * conv_prod:
        raise ValueError("prop_local: W / out do not match the gather table")
    check(lib().snn_prop_local_f32(_ptr(W, F32), _ptr(src, torch.int32), _ptr(s, "spike"), _ptr(out, F32), B, Cin, n_filters,
                                   conv_prod, kernel_prod, n_src, int(accumulate), _stream()), "prop_local")
    return out


def local_postpre(W, src, s_src, x_src, s_tgt, x_tgt, nu0, nu1, n_filters, decay=1.0, wmin=None, wmax=None, reduce="sum"):
    """f5: PostPre on LocalConnection1D/2D/3D weights (learning.py:208-389); s_src / x_src [B, n_src], s_tgt / x_tgt
    [B, F*conv_prod]."""
    B = s_src.shape[0]
    Cin, conv_prod, kernel_prod = src.shape
    n_src = s_src.numel() // B
    if tuple(W.shape) != (Cin, n_filters * conv_prod, kernel_prod) or x_src.numel() != B * n_src \
            or s_tgt.numel() != B * n_filters * conv_prod or x_tgt.numel() != s_tgt.numel():
        raise ValueError("local_postpre: operand shapes do not match the gather table")
    if _reduce(reduce):
        check(lib().snn_local_postpre_red(_ptr(W, F32), _ptr(src, torch.int32), _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"),
                                          _ptr(x_tgt, F32), B, Cin, n_filters, conv_prod, kernel_prod, n_src, float(nu0), float(nu1),
                                          float(decay), *_bounds(wmin, wmax), _reduce(reduce), _stream()), "local_postpre_red")
        return
    check(lib().snn_local_postpre(_ptr(W, F32), _ptr(src, torch.int32), _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"),
                                  _ptr(x_tgt, F32), B, Cin, n_filters, conv_prod, kernel_prod, n_src, float(nu0), float(nu1),
                                  float(decay), *_bounds(wmin, wmax), _stream()), "local_postpre")


def prop_convnd(W, s, out, bias=None, stride=1, pad=0, accumulate=False):
    """f6: Conv1dConnection / Conv3dConnection.compute (F.conv1d / F.conv3d on 0/1 spikes); W [Cout, Cin, K] with s [B, Cin, N],
    or W [Cout, Cin, KD, KH, KW] with s [B, Cin, D, H, W]; out [B, Cout, *positions]."""
    B, Cin = s.shape[0], s.shape[1]
    Cout = W.shape[0]
    if W.dim() == 3 and s.dim() == 3:
        (D, H, Wd), (KD, KH, KW) = (1, 1, s.shape[2]), (1, 1, W.shape[2])
    elif W.dim() == 5 and s.dim() == 5:
        (D, H, Wd), (KD, KH, KW) = s.shape[2:], W.shape[2:]
    else:
        raise ValueError("prop_convnd: W [Cout, Cin, K] with s [B, Cin, N], or W [Cout, Cin, KD, KH, KW] with s [B, Cin, D, H, W]")
    if W.shape[1] != Cin:
        raise ValueError("prop_convnd: W and s disagree on the input channels")
    pads = (0 if (D, KD) == (1, 1) else pad, 0 if (H, KH) == (1, 1) else pad, pad)   # (a unit axis is not padded: snnhip.h)
    P = 1
    for n, k, q in zip((D, H, Wd), (KD, KH, KW), pads):
        P *= (n + 2 * q - k) // stride + 1
    if out.numel() != B * Cout * P:
        raise ValueError("prop_convnd: out does not hold [B, Cout, *positions]")
    check(lib().snn_prop_convnd_f32(_ptr(W, F32), _ptr(bias, F32, True), _ptr(s, "spike"), _ptr(out, F32), B, Cin, D, H, Wd, Cout,
                                    KD, KH, KW, int(stride), int(pad), int(accumulate), _stream()), "prop_convnd")
    return out


def convnd_postpre(W, pp_src, s_src, x_src, s_tgt, x_tgt, nu0, nu1, decay=1.0, wmin=None, wmax=None, ws=None, reduce="sum"):
    """f6: PostPre on Conv1dConnection / Conv3dConnection weights [Cout, Cin, *kernel] (learning.py:422-455 / :499-559);
    pp_src int32 [L, Cin*K] (the connection's gather table), s_src / x_src [B, n_src], s_tgt / x_tgt [B, Cout*L]."""
    B = s_src.shape[0]
    L, J = pp_src.shape
    Cout = W.shape[0]
    n_src = s_src.numel() // B
    if W.numel() != Cout * J or x_src.numel() != B * n_src or s_tgt.numel() != B * Cout * L or x_tgt.numel() != s_tgt.numel():
        raise ValueError("convnd_postpre: operand shapes do not match the gather table")
    if ws is None:
        ws = torch.empty(B * Cout * ((L + 31) // 32), dtype=torch.int32, device=W.device)
    if _reduce(reduce):
        check(lib().snn_convnd_postpre_red(_ptr(W, F32), _ptr(pp_src, torch.int32), _ptr(s_src, "spike"), _ptr(x_src, F32),
                                           _ptr(s_tgt, "spike"), _ptr(x_tgt, F32), B, Cout, L, J, n_src, float(nu0), float(nu1), float(decay),
                                           *_bounds(wmin, wmax), _ptr(ws, torch.int32), _reduce(reduce), _stream()), "convnd_postpre_red")
        return
    check(lib().snn_convnd_postpre(_ptr(W, F32), _ptr(pp_src, torch.int32), _ptr(s_src, "spike"), _ptr(x_src, F32),
                                   _ptr(s_tgt, "spike"), _ptr(x_tgt, F32), B, Cout, L, J, n_src, float(nu0), float(nu1), float(decay),
                                   *_bounds(wmin, wmax), _ptr(ws, torch.int32), _stream()), "convnd_postpre")


def sparse_compile(w):
    """f9: the compiled form of a sparse COO matrix `w` [Nin, N] for snn_prop_sparse_f32 (include/snnhip.h), on w's device:
    (ptr int32 [ceil(N/256) * Nin + 1], col uint8 [nnz], val float32 [nnz]).  `w` is coalesced first; every stored entry is kept."""
    if not w.is_sparse or w.dim() != 2 or w.dtype != F32:
        raise ValueError("sparse_compile: a 2-D float32 sparse COO tensor is required")
    wc = w.detach().coalesce()                      # entries in (i, j) ascending order, duplicates summed
    Nin, N = wc.shape
    TJ = _lib.SPARSE_TJ
    tiles = (N + TJ - 1) // TJ
    nnz = wc._nnz()
    if nnz >= 2 ** 31 or Nin > 2 ** 24 or tiles * Nin + 1 > 2 ** 31 - 1:
        raise NotImplementedError(f"bindsnet_amd: a sparse [{Nin}, {N}] matrix with {nnz} entries exceeds the int32 indices of "
                                  "snn_prop_sparse_f32 (nnz < 2^31, Nin <= 2^24, ceil(N/256) * Nin < 2^31 - 1)")
    i, j = wc.indices()
    key = torch.div(j, TJ, rounding_mode="floor") * Nin + i
    order = torch.sort(key, stable=True).indices    # tile-major; inside a tile the coalesced (i, j) order stays
    ptr = torch.zeros(tiles * Nin + 1, dtype=torch.int64, device=wc.device)
    ptr[1:] = torch.cumsum(torch.bincount(key, minlength=tiles * Nin), 0)
    return ptr.to(torch.int32), (j[order] % TJ).to(torch.uint8).contiguous(), wc.values()[order].contiguous()


def prop_sparse(compiled, s, out, bias=None, accumulate=False):
    """f9: out (+)= s @ w (+ b) for the sparse `w` that `compiled` = sparse_compile(w) holds: per column the stored entries of
    the spiking sources in ascending order, one rounded f32 add each, the bias last."""
    ptr, col, val = compiled
    B = s.shape[0]
    Nin, N = s.numel() // B, out.numel() // B
    tiles = (N + _lib.SPARSE_TJ - 1) // _lib.SPARSE_TJ
    if s.numel() != B * Nin or out.numel() != B * N or ptr.numel() != tiles * Nin + 1 or col.numel() != val.numel():
        raise ValueError("prop_sparse: the compiled form does not belong to a matrix of these shapes")
    if bias is not None and bias.numel() != N:
        raise ValueError("prop_sparse: bias must have one entry per target")
    nnz = val.numel()
    check(lib().snn_prop_sparse_f32(_ptr(ptr, torch.int32), _ptr(col, torch.uint8) if nnz else None, _ptr(val, F32) if nnz else None,
                                    nnz, _ptr(bias, F32, True), _ptr(s, "spike"), _ptr(out, F32), B, Nin, N, int(accumulate),
                                    _stream()), "prop_sparse")
    return out


def _pv(vectors, N):
    """The snn_pervec argument of a *_pv entry point from {quantity: f32 [N] device tensor} (None / empty: a null pointer,
    the scalar step).  Returns (argument, the struct to keep alive over the call)."""
    if not vectors:
        return None, None
    for name, t in vectors.items():
        if t.numel() != N:
            raise ValueError(f"per-neuron `{name}` has {t.numel()} entries, the layer {N} neurons")
        _ptr(t, F32)
    pv = _lib.pervec(vectors)
    return C.byref(pv), pv


def pool_geometry(spatial, kernel_size, stride, padding, dilation):
    """f11: the five int[3] arrays of snn_prop_pool_f32 for a pooling of rank len(spatial) <= 3 (the missing leading dimensions:
    size 1, kernel 1, stride 1, padding 0, dilation 1) and the pooled sizes, out = (in + 2p - d(k - 1) - 1) // s + 1."""
    nd = len(spatial)
    tup = lambda v: tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v),) * nd       # noqa: E731
    fields = [tuple(int(x) for x in spatial), tup(kernel_size), tup(stride), tup(padding), tup(dilation)]
    if nd < 1 or nd > 3 or any(len(f) != nd for f in fields):
        raise ValueError(f"pool_geometry: {nd} spatial dimensions need {nd} entries (or one int) per field")
    unit = (1, 1, 1, 0, 1)
    arrays = [(C.c_int * 3)(*((u,) * (3 - nd) + f)) for u, f in zip(unit, fields)]
    out = tuple((i + 2 * p - d * (k - 1) - 1) // s + 1 for i, k, s, p, d in zip(*fields))
    return arrays, out


def prop_pool(fr, s, out, kernel_size, stride=1, padding=0, dilation=1, decay=0.0, accumulate=False):
    """f11: one MaxPoolNdConnection.compute: fr [B, C, *spatial] <- fr - decay * fr + s; out [B, C, *pooled] (+)= s gathered at
    the indices of F.max_poolNd(fr, ..., return_indices=True)."""
    if fr.dim() < 3 or fr.dim() > 5 or tuple(s.shape) != tuple(fr.shape):
        raise ValueError("prop_pool: firing rates and spikes must both be [B, C, *spatial] with 1 to 3 spatial dimensions")
    arrays, pooled = pool_geometry(fr.shape[2:], kernel_size, stride, padding, dilation)
    if min(pooled) <= 0 or tuple(out.shape) != tuple(fr.shape[:2]) + pooled:
        raise ValueError(f"prop_pool: out must be {tuple(fr.shape[:2]) + pooled}, got {tuple(out.shape)}")
    check(lib().snn_prop_pool_f32(_ptr(fr, F32), _ptr(s, "spike"), _ptr(out, F32), fr.shape[0], fr.shape[1], *arrays, float(decay),
                                  int(accumulate), _stream()), "prop_pool")
    return out


def avgpool_geometry(plane, kernel_size, stride=None, padding=0, ceil_mode=False):
    """f18: the four int[2] arrays of snn_prop_avgpool2d_f32 and the pooled sizes as ATen's avg_pool2d computes them (stride None:
    the kernel's; with ceil_mode a last window that would start in the right padding is dropped)."""
    pair = lambda v: tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v),) * 2       # noqa: E731
    k = pair(kernel_size)
    fields = [tuple(int(x) for x in plane), k, k if stride is None or stride == [] or stride == () else pair(stride), pair(padding)]
    if any(len(f) != 2 for f in fields):
        raise ValueError("avgpool_geometry: the plane, kernel_size, stride and padding need two entries (or one int) each")
    if min(fields[2]) <= 0 or min(k) <= 0:
        raise ValueError("avgpool_geometry: kernel_size and stride must be positive")
    out = []
    for i, kk, s, p in zip(*fields):
        o = (i + 2 * p - kk + (s - 1 if ceil_mode else 0)) // s + 1
        out.append(o - 1 if ceil_mode and (o - 1) * s >= i + p else o)
    return [(C.c_int * 2)(*f) for f in fields], tuple(out)


def prop_avgpool(s, out, kernel_size, stride=None, padding=0, ceil_mode=False, count_include_pad=True, divisor_override=None,
                 accumulate=False):
    """f18: one AvgPool2dConnection.compute: out [B, C, OH, OW] (+)= F.avg_pool2d(s.float(), ...) for spike bytes s [B, C, H, W], every
    window an integer count divided once (include/snnhip.h)."""
    if s.dim() != 4:
        raise ValueError("prop_avgpool: spikes must be [B, C, H, W]")
    if divisor_override is not None and int(divisor_override) == 0:
        raise ValueError("prop_avgpool: divisor_override must not be zero (torch: divisor must be not zero)")
    arrays, pooled = avgpool_geometry(s.shape[2:], kernel_size, stride, padding, ceil_mode)
    if min(pooled) <= 0 or tuple(out.shape) != tuple(s.shape[:2]) + pooled:
        raise ValueError(f"prop_avgpool: out must be {tuple(s.shape[:2]) + pooled}, got {tuple(out.shape)}")
    check(lib().snn_prop_avgpool2d_f32(_ptr(s, "spike"), _ptr(out, F32), s.shape[0], s.shape[1], *arrays, int(bool(ceil_mode)),
                                       int(bool(count_include_pad)), 0 if divisor_override is None else int(divisor_override),
                                       int(accumulate), _stream()), "prop_avgpool")
    return out


def prop_meanfield(w, s, out, accumulate=False, store=False):
    """f11: MeanFieldConnection.compute: out [B, n_tgt] (+)= s.float().mean() * w, the mean over the whole of s [B, n_src]; `w` has
    one element or a shape that is a tail of out's.  store: out = mean * w itself (a zero keeps its sign) instead of 0 + mean * w."""
    B = s.shape[0]
    if s.numel() > _lib.MEANFIELD_MAX:
        raise NotImplementedError(f"bindsnet_amd: MeanFieldConnection over {s.numel()} source elements (batch x source.n) is not "
                                  f"supported: f32(count) / f32(numel) is the reference's mean up to 2^24 elements")
    if out.shape[0] != B or w.numel() < 1 or out.numel() % w.numel() != 0:
        raise ValueError("prop_meanfield: out must be [B, ...] and w's element count must divide out's")
    mode = _lib.MEANFIELD_STORE if store else int(accumulate)
    check(lib().snn_prop_meanfield_f32(_ptr(w, F32), w.numel(), _ptr(s, "spike"), _ptr(out, F32), B, s.numel() // B, out.numel() // B,
                                       mode, _stream()), "prop_meanfield")
    return out


def record_segments(pairs, t: int):
    """Monitor.record() for float state, one launch (snn_record_segments): for every (src, dst) of `pairs` -- contiguous float32
    device tensors, dst holding a whole number of src-sized slices, [T, *src.shape] -- slice `t` of dst becomes a bit copy of src.
    A src must not overlap the slice it is copied to."""
    pairs = list(pairs)
    arr = (_lib.RecordSegment * max(1, len(pairs)))()
    for k, (src, dst) in enumerate(pairs):
        n = src.numel()
        if n == 0 or dst.numel() % n or not 0 <= t < dst.numel() // n:
            raise ValueError(f"record_segments: pair {k}: dst must hold whole slices of src's size and 0 <= t < their number "
                             f"(src {tuple(src.shape)}, dst {tuple(dst.shape)}, t = {t})")
        arr[k].src, arr[k].dst, arr[k].bytes = _ptr(src, F32).value, _ptr(dst, F32).value, 4 * n
    check(lib().snn_record_segments(arr, len(pairs), t, _stream()), "record_segments")


def input_step(s, x=None, trace_decay=0.0, trace_scale=1.0, additive=False, raster=None, pv=None):
    """pv (here and in every step below): optional {quantity name (_lib.PERVEC): f32 [N] device tensor} of per-neuron
    parameters that take the place of the scalars (include/snnhip.h f10)."""
    if pv:
        B = s.shape[0]
        arg, _keep = _pv(pv, s.numel() // B)
        check(lib().snn_input_step_pv(_ptr(s, "spike"), _ptr(x, F32, True), B, s.numel() // B, trace_decay, trace_scale,
                                      int(additive), arg, _ptr(raster, "spike", True), _stream()), "input_step")
        return
    check(lib().snn_input_step(_ptr(s, "spike"), _ptr(x, F32, True), s.numel(), trace_decay, trace_scale,
                               int(additive), _ptr(raster, "spike", True), _stream()), "input_step")


def lif_step(v, refrac, s, x, I, p: LifParams, raster_s=None, raster_v=None, thresh_vec=None, pv=None):
    """thresh_vec: optional f32 [N] per-neuron thresholds (replace p.thresh; nodes.py:425-498 with a tensor-valued `thresh`)."""
    B = v.shape[0]
    N = v.numel() // B
    if pv:
        if thresh_vec is not None:
            pv = dict(pv, thresh=thresh_vec)
        arg, _keep = _pv(pv, N)
        check(lib().snn_lif_step_pv(_ptr(v, F32), _ptr(refrac, F32), _ptr(s, "spike"), _ptr(x, F32, True), _ptr(I, F32), B, N,
                                    C.byref(p), arg, _ptr(raster_s, "spike", True), _ptr(raster_v, F32, True), _stream()), "lif_step")
        return
    if thresh_vec is not None and thresh_vec.numel() != N:
        raise ValueError(f"thresh_vec has {thresh_vec.numel()} entries, the layer {N} neurons")
    check(lib().snn_lif_step_vth(_ptr(v, F32), _ptr(refrac, F32), _ptr(s, "spike"), _ptr(x, F32, True), _ptr(I, F32), B, N,
                                 C.byref(p), _ptr(thresh_vec, F32, True), _ptr(raster_s, "spike", True), _ptr(raster_v, F32, True), _stream()),
          "lif_step")


def _node_args(v):
    B = v.shape[0]
    return B, v.numel() // B


def mcp_step(v, s, x, I, p: LifParams, raster_s=None, raster_v=None, pv=None):
    """McCullochPitts.forward (nodes.py:278-288): v = I, s = v >= thresh, trace."""
    B, N = _node_args(v)
    arg, _keep = _pv(pv, N)
    check(lib().snn_mcp_step_pv(_ptr(v, F32), _ptr(s, "spike"), _ptr(x, F32, True), _ptr(I, F32), B, N, C.byref(p), arg,
                                _ptr(raster_s, "spike", True), _ptr(raster_v, F32, True), _stream()), "mcp_step")


def if_step(v, refrac, s, x, I, p: LifParams, raster_s=None, raster_v=None, pv=None):
    """IFNodes.forward (nodes.py:371-395)."""
    B, N = _node_args(v)
    arg, _keep = _pv(pv, N)
    check(lib().snn_if_step_pv(_ptr(v, F32), _ptr(refrac, F32), _ptr(s, "spike"), _ptr(x, F32, True), _ptr(I, F32), B, N, C.byref(p), arg,
                               _ptr(raster_s, "spike", True), _ptr(raster_v, F32, True), _stream()), "if_step")


def boosted_step(v, refrac, s, x, I, p: LifParams, raster_s=None, raster_v=None, pv=None):
    """BoostedLIFNodes.forward (nodes.py:621-648); I is masked in place where refractory."""
    B, N = _node_args(v)
    arg, _keep = _pv(pv, N)
    check(lib().snn_boosted_step_pv(_ptr(v, F32), _ptr(refrac, F32), _ptr(s, "spike"), _ptr(x, F32, True), _ptr(I, F32), B, N,
                                    C.byref(p), arg, _ptr(raster_s, "spike", True), _ptr(raster_v, F32, True), _stream()), "boosted_step")


def clif_step(v, refrac, i, s, x, I, p: LifParams, i_decay, raster_s=None, raster_v=None, pv=None):
    """CurrentLIFNodes.forward (nodes.py:762-791); i [B,N] is the synaptic current."""
    B, N = _node_args(v)
    arg, _keep = _pv(pv, N)
    check(lib().snn_clif_step_pv(_ptr(v, F32), _ptr(refrac, F32), _ptr(i, F32), _ptr(s, "spike"), _ptr(x, F32, True), _ptr(I, F32), B, N,
                                 C.byref(p), i_decay, arg, _ptr(raster_s, "spike", True), _ptr(raster_v, F32, True), _stream()), "clif_step")


def srm0_step(rng_state, v, refrac, s, x, I, s_prob, rho, p: LifParams, eps_0, rho_0, d_thresh, raster_s=None, raster_v=None, pv=None):
    """SRM0Nodes.forward (nodes.py:1639-1671), the draw included.  rng_state: the int32 image of a device generator state
    (rng.DeviceGenerator.state) holding the HOST generator; it is advanced in place by B * N 32-bit outputs.  s_prob, rho: f32
    [B, N] outputs."""
    B, N = _node_args(v)
    arg, _keep = _pv(pv, N)
    if s_prob.numel() != B * N or rho.numel() != B * N or I.numel() != B * N:
        raise ValueError("srm0_step: I, s_prob and rho must have the shape of v")
    check(lib().snn_srm0_step_pv(_ptr(rng_state, torch.int32), _ptr(v, F32), _ptr(refrac, F32), _ptr(s, "spike"), _ptr(x, F32, True),
                                 _ptr(I, F32), _ptr(s_prob, F32), _ptr(rho, F32), B, N, C.byref(p), eps_0, rho_0, d_thresh, arg,
                                 _ptr(raster_s, "spike", True), _ptr(raster_v, F32, True), _stream()), "srm0_step")


def rmax_step(W, e_trace, s_tgt, s_prob, x_src, reward, nu0, dt, tc_c, tc_e, wdecay=1.0, wmin=None, wmax=None):
    """Rmax._connection_update (learning.py:2923-2960), batch 1: W, e_trace [Nin, N]; s_tgt, s_prob [N]; x_src [Nin]."""
    Nin, N = W.shape
    if e_trace.numel() != Nin * N or s_tgt.numel() != N or s_prob.numel() != N or x_src.numel() != Nin:
        raise ValueError("rmax_step: operand sizes do not match the weights")
    check(lib().snn_rmax_step(_ptr(W, F32), _ptr(e_trace, F32), _ptr(s_tgt, "spike"), _ptr(s_prob, F32), _ptr(x_src, F32), Nin, N,
                              reward, nu0, dt, tc_c, tc_e, wdecay, *_bounds(wmin, wmax), _stream()), "rmax_step")


def prop_window(W, ring, head, s, out, bias=None, accumulate=False):
    """Connection.compute_window (topology.py:348-374) on a ring: ring u8 [B, Wres, Nin] with its oldest entry in physical slot
    `head`; the call overwrites that slot with s [B, Nin] and writes out [B, Wres, N] (+)= window @ W (+ b), slot 0 the oldest,
    each sum over the spiking sources in ascending order.  The caller's next head is (head + 1) % Wres."""
    B, Wres, Nin = ring.shape
    N = W.shape[1]
    if W.shape[0] != Nin or s.numel() != B * Nin or out.numel() != B * Wres * N or not 0 <= head < Wres:
        raise ValueError("prop_window: operand sizes do not match")
    check(lib().snn_prop_window_f32(_ptr(W, F32), _ptr(bias, F32, True), _ptr(ring, torch.uint8), int(head), _ptr(s, "spike"),
                                    _ptr(out, F32), B, Wres, Nin, N, int(accumulate), _stream()), "prop_window")
    return out


def csrm_step(v, s, x, theta, xwin, last, resK, refK, p, raster_s=None, raster_v=None, pv=None):
    """CSRMNodes.forward (nodes.py:1427-1464) in one launch: xwin f32 [B, Wres, N] the window of currents, last f32 [B, Wref, N]
    the layer's last spikes (shifted in place, the new spikes appended), resK / refK the kernels, p an snn_dc_params."""
    B, N = _node_args(v)
    arg, _keep = _pv(pv, N)
    Wres, Wref = resK.numel(), refK.numel()
    if xwin.numel() != B * Wres * N or last.numel() != B * Wref * N or theta.numel() != N:
        raise ValueError("csrm_step: xwin, last and theta must be [B, Wres, N], [B, Wref, N] and [N]")
    check(lib().snn_csrm_step(_ptr(v, F32), _ptr(s, "spike"), _ptr(x, F32, True), _ptr(theta, F32), _ptr(xwin, F32), _ptr(last, F32),
                              _ptr(resK, F32), Wres, _ptr(refK, F32), Wref, B, N, C.byref(p), arg, _ptr(raster_s, "spike", True),
                              _ptr(raster_v, F32, True), _stream()), "csrm_step")


def sif_step(v, refrac, s, x, I, p: LifParams, summed=None, raster_s=None, raster_v=None, pv=None):
    """f14: SubtractiveResetIFNodes.forward (conversion/nodes.py:73-99); summed f32 [B, N] (sum_input) takes the raw input."""
    B, N = _node_args(v)
    arg, _keep = _pv(pv, N)
    if I.numel() != B * N or (summed is not None and summed.numel() != B * N):
        raise ValueError("sif_step: the input and `summed` must have the layer's [B, N] elements")
    check(lib().snn_sif_step_pv(_ptr(v, F32), _ptr(refrac, F32), _ptr(s, "spike"), _ptr(x, F32, True), _ptr(summed, F32, True), _ptr(I, F32),
                                B, N, C.byref(p), arg, _ptr(raster_s, "spike", True), _ptr(raster_v, F32, True), _stream()), "sif_step")


def pass_step(s, I, raster_s=None):
    """f14: PassThroughNodes.forward (conversion/nodes.py:161-169) with the spikes kept as bytes: s [B, N] = (I != 0)."""
    B = s.shape[0]
    if I.numel() != s.numel():
        raise ValueError("pass_step: the input must have the layer's [B, N] elements")
    check(lib().snn_pass_step(_ptr(s, "spike"), _ptr(I, F32), B, s.numel() // B, _ptr(raster_s, "spike", True), _stream()), "pass_step")


def gather_geometry(src_shape, out_shape, strides, offsets):
    """f14: the four int[3] arrays of snn_prop_gather_f32 (output extents, source extents in the output's order, source strides,
    leading offsets) for a gather of rank <= 3; missing leading dimensions are 1 / 1 / 0 / 0."""
    nd = len(out_shape)
    fields = [tuple(int(v) for v in f) for f in (out_shape, src_shape, strides, offsets)]
    if nd < 1 or nd > 3 or any(len(f) != nd for f in fields):
        raise ValueError("gather_geometry: one to three dimensions, the same number in every field")
    return [(C.c_int * 3)(*((u,) * (3 - nd) + f)) for u, f in zip((1, 1, 0, 0), fields)]


def permute_geometry(src_shape, dims):
    """The gather of `s.permute(0, *[d + 1 for d in dims])` over a sample of shape src_shape: (arrays, permuted shape)."""
    src_shape = tuple(int(v) for v in src_shape)
    row_major = [1] * len(src_shape)
    for a in range(len(src_shape) - 2, -1, -1):
        row_major[a] = row_major[a + 1] * src_shape[a + 1]
    out = tuple(src_shape[d] for d in dims)
    return gather_geometry(out, out, [row_major[d] for d in dims], (0,) * len(dims)), out


def pad_geometry(src_shape, before, after):
    """The gather of a zero padding of `before[a]` / `after[a]` elements around every dimension of a sample: (arrays, padded shape)."""
    src_shape = tuple(int(v) for v in src_shape)
    row_major = [1] * len(src_shape)
    for a in range(len(src_shape) - 2, -1, -1):
        row_major[a] = row_major[a + 1] * src_shape[a + 1]
    out = tuple(n + int(b) + int(e) for n, b, e in zip(src_shape, before, after))
    return gather_geometry(src_shape, out, row_major, before), out


def prop_gather(s, out, arrays, accumulate=False):
    """f14: PermuteConnection / ConstantPad2dConnection.compute: out f32 [B, *out shape] (+)= float(s[b, gathered index]), 0 in the
    padding; `arrays` from permute_geometry / pad_geometry."""
    B = s.shape[0]
    n_out = arrays[0][0] * arrays[0][1] * arrays[0][2]
    if out.shape[0] != B or out.numel() != B * n_out:
        raise ValueError(f"prop_gather: out must hold [{B}, {n_out}] elements, got {tuple(out.shape)}")
    check(lib().snn_prop_gather_f32(_ptr(s, "spike"), _ptr(out, F32), B, s.numel() // B, *arrays, int(accumulate), _stream()), "prop_gather")
    return out


def izh_step(v, u, s, x, I, a, b, c, d, St, p: LifParams, raster_s=None, raster_v=None, pv=None):
    """IzhikevichNodes.forward (nodes.py:1265-1296) in one launch; s holds the previous step's spikes at entry; St is the
    lateral matrix transposed ([N, N], St[i, j] = S[j, i]); the lateral sum is added to I in place."""
    B, N = _node_args(v)
    if St.numel() != N * N or any(t.numel() != N for t in (a, b, c, d)):
        raise ValueError(f"a, b, c, d must have {N} entries and St {N} x {N}")
    if N > _lib.IZH_MAX_N:
        raise NotImplementedError(f"bindsnet_amd: IzhikevichNodes of more than {_lib.IZH_MAX_N} neurons")
    arg, _keep = _pv(pv, N)
    check(lib().snn_izh_step_pv(_ptr(v, F32), _ptr(u, F32), _ptr(s, "spike"), _ptr(x, F32, True), _ptr(I, F32), _ptr(a, F32), _ptr(b, F32),
                                _ptr(c, F32), _ptr(d, F32), _ptr(St, F32), B, N, C.byref(p), arg, _ptr(raster_s, "spike", True),
                                _ptr(raster_v, F32, True), _stream()), "izh_step")


def dc_step(v, refrac, s, x, theta, I, p: DcParams, noise_q, cursor, status, raster_s=None, raster_v=None, pv=None):
    """cursor: int64[2] device tensor ([0] running count, [1] scratch); status: int32[1]."""
    B = v.shape[0]
    N = v.numel() // B
    qlen = 0 if noise_q is None else noise_q.numel()
    arg, _keep = _pv(pv, N)
    check(lib().snn_dc_step_pv(_ptr(v, F32), _ptr(refrac, F32), _ptr(s, "spike"), _ptr(x, F32, True), _ptr(theta, F32),
                               _ptr(I, F32), B, N, C.byref(p), arg, _ptr(noise_q, F32, True), qlen,
                               _ptr(cursor, torch.int64, True), _ptr(status, torch.int32, True),
                               _ptr(raster_s, "spike", True), _ptr(raster_v, F32, True), _stream()), "dc_step")


def dc_arbitrate(s, x, p: DcParams, noise_q, cursor, status, raster_s=None):
    """The second half of dc_step on its own (nodes.py:1097-1111): one_spike winners on the crossings `s` [B,N] (in place),
    trace, raster.  cursor[1] = offset of this step's first draw in noise_q (rng_fill_exponential leaves 0 and the draws
    in its qbuf)."""
    B = s.shape[0]
    N = s.numel() // B
    qlen = 0 if noise_q is None else noise_q.numel()
    check(lib().snn_dc_arbitrate(_ptr(s, "spike"), _ptr(x, F32, True), B, N, C.byref(p), _ptr(noise_q, F32, True), qlen,
                                 _ptr(cursor, torch.int64, True), _ptr(status, torch.int32, True),
                                 _ptr(raster_s, "spike", True), _stream()), "dc_arbitrate")


def stdp_postpre(W, s_src, x_src, s_tgt, x_tgt, nu0, nu1, use_dt, dt=1.0, decay=1.0, wmin=None, wmax=None,
                 assume_clamped=False, reduce="sum"):
    """a8 / a9: PostPre on a dense or MCC weight matrix.  reduce: the batch reduction, "sum" (the entry points as they were), "mean",
    "amax" or "amin" (the *_red entry points, include/snnhip.h f15)."""
    B = s_src.shape[0]
    Nin, N = W.shape
    if W.dtype in HALF:                 # (every element is visited: assume_clamped has nothing to skip)
        check(lib().snn_stdp_postpre_h16_red(_ptr(W, W.dtype), HALF[W.dtype], _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"),
                                             _ptr(x_tgt, F32), B, Nin, N, nu0, nu1, int(use_dt), dt, decay, *_bounds(wmin, wmax),
                                             _reduce(reduce), _stream()), "stdp_postpre_h16")
        return
    # the entry point chooses the instance: another batch reduction, per-synapse rates / bounds (include/snnhip.h f13), or the scalar kernel
    nu0, nu1, bounds, sp, _keep = _syn(W, nu0, nu1, wmin, wmax)
    check(lib().snn_stdp_postpre_red(_ptr(W, F32), _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"), _ptr(x_tgt, F32),
                                     B, Nin, N, nu0, nu1, int(use_dt), dt, decay, *bounds, int(assume_clamped),
                                     None if sp is None else C.byref(sp), _reduce(reduce), _stream()), "stdp_postpre")


def mstdp_step(W, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, reward, nu0, a_plus, a_minus,
               decay_plus, decay_minus, wdecay=1.0, wmin=None, wmax=None, reward_vec=None, reduce="sum"):
    B = s_src.shape[0]
    Nin, N = W.shape
    nu0, _, bounds, sp, _keep = _syn(W, nu0, 0.0, wmin, wmax)
    check(lib().snn_mstdp_step_red(_ptr(W, F32), _ptr(p_plus, F32), _ptr(p_minus, F32), _ptr(s_src_prev, "spike"),
                                   _ptr(s_tgt_prev, "spike"), _ptr(s_src, "spike"), _ptr(s_tgt, "spike"), B, Nin, N,
                                   reward, _ptr(reward_vec, F32, True), nu0, a_plus, a_minus, decay_plus, decay_minus,
                                   wdecay, *bounds, None if sp is None else C.byref(sp), _reduce(reduce), _stream()), "mstdp_step")


def conv2d_postpre(W, s_src, x_src, s_tgt, x_tgt, nu0, nu1, stride=1, pad=0, decay=1.0, wmin=None, wmax=None, ws=None, reduce="sum"):
    """f4: PostPre on Conv2dConnection weights [Cout,Cin,KH,KW]; s_src / x_src [B,Cin,H,W], s_tgt / x_tgt [B,Cout,OH,OW]."""
    B, Cin, H, Wd = s_src.shape
    Cout, _, KH, KW = W.shape
    if ws is None:
        ws = torch.empty(2 * B * W.numel(), dtype=F32, device=W.device)
    if _reduce(reduce):
        check(lib().snn_conv2d_postpre_red(_ptr(W, F32), _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"), _ptr(x_tgt, F32),
                                           B, Cin, H, Wd, Cout, KH, KW, stride, pad, nu0, nu1, decay, *_bounds(wmin, wmax),
                                           _ptr(ws, F32), _reduce(reduce), _stream()), "conv2d_postpre_red")
        return
    check(lib().snn_conv2d_postpre(_ptr(W, F32), _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"), _ptr(x_tgt, F32),
                                   B, Cin, H, Wd, Cout, KH, KW, stride, pad, nu0, nu1, decay, *_bounds(wmin, wmax),
                                   _ptr(ws, F32), _stream()), "conv2d_postpre")


def conv2d_hebbian(W, s_src, x_src, s_tgt, x_tgt, nu0, nu1, weight_dependent=False, stride=1, pad=0, decay=1.0, wmin=None, wmax=None,
                   ws=None, reduce="sum"):
    """f4: Hebbian (weight_dependent=False) / WeightDependentPostPre (True) on Conv2dConnection weights; shapes as conv2d_postpre."""
    B, Cin, H, Wd = s_src.shape
    Cout, _, KH, KW = W.shape
    if ws is None:
        ws = torch.empty(2 * B * W.numel(), dtype=F32, device=W.device)
    if _reduce(reduce):
        check(lib().snn_conv2d_hebbian_red(_ptr(W, F32), _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"), _ptr(x_tgt, F32),
                                           B, Cin, H, Wd, Cout, KH, KW, stride, pad, nu0, nu1, int(weight_dependent), decay,
                                           *_bounds(wmin, wmax), _ptr(ws, F32), _reduce(reduce), _stream()), "conv2d_hebbian_red")
        return
    check(lib().snn_conv2d_hebbian(_ptr(W, F32), _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"), _ptr(x_tgt, F32),
                                   B, Cin, H, Wd, Cout, KH, KW, stride, pad, nu0, nu1, int(weight_dependent), decay,
                                   *_bounds(wmin, wmax), _ptr(ws, F32), _stream()), "conv2d_hebbian")


def conv2d_mstdp_step(W, elig, p_plus, p_minus, s_src, s_tgt, reward, nu0, a_plus, a_minus, decay_plus, decay_minus, stride=1, pad=0,
                      wdecay=1.0, wmin=None, wmax=None):
    """f4: MSTDP on Conv2dConnection weights [Cout,Cin,KH,KW] at batch 1; elig like W, p_plus [Cin,H,W], p_minus [Cout,OH*OW],
    s_src [Cin,H,W], s_tgt [Cout,OH,OW] (a leading batch dimension of 1 is fine)."""
    Cin, H, Wd = s_src.shape[-3:]
    Cout, _, KH, KW = W.shape
    check(lib().snn_conv2d_mstdp_step(_ptr(W, F32), _ptr(elig, F32), _ptr(p_plus, F32), _ptr(p_minus, F32), _ptr(s_src, "spike"),
                                      _ptr(s_tgt, "spike"), Cin, H, Wd, Cout, KH, KW, stride, pad, reward, nu0, a_plus, a_minus,
                                      decay_plus, decay_minus, wdecay, *_bounds(wmin, wmax), _stream()), "conv2d_mstdp_step")


def stdp_hebbian(W, s_src, x_src, s_tgt, x_tgt, nu0, nu1, weight_dependent=False, decay=1.0, wmin=None, wmax=None, reduce="sum"):
    """f3: Hebbian (weight_dependent=False) / WeightDependentPostPre (True) on a dense weight matrix."""
    B = s_src.shape[0]
    Nin, N = W.shape
    nu0, nu1, bounds, sp, _keep = _syn(W, nu0, nu1, wmin, wmax)
    check(lib().snn_stdp_hebbian_red(_ptr(W, F32), _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"), _ptr(x_tgt, F32),
                                     B, Nin, N, nu0, nu1, int(weight_dependent), decay, *bounds, None if sp is None else C.byref(sp),
                                     _reduce(reduce), _stream()), "stdp_hebbian")


def mstdpet_step(W, e_trace, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, reward, nu0, dt, a_plus, a_minus,
                 decay_plus, decay_minus, decay_e, tc_e, wdecay=1.0, wmin=None, wmax=None):
    Nin, N = W.shape
    nu0, _, bounds, sp, _keep = _syn(W, nu0, 0.0, wmin, wmax)
    check(lib().snn_mstdpet_step_pv(_ptr(W, F32), _ptr(e_trace, F32), _ptr(p_plus, F32), _ptr(p_minus, F32), _ptr(s_src_prev, "spike"),
                                    _ptr(s_tgt_prev, "spike"), _ptr(s_src, "spike"), _ptr(s_tgt, "spike"), Nin, N, reward, nu0, dt,
                                    a_plus, a_minus, decay_plus, decay_minus, decay_e, tc_e, wdecay, *bounds,
                                    None if sp is None else C.byref(sp), _stream()), "mstdpet_step")


def _ring(ring, W, K):
    """A time-averaging ring as the *_avg_step entry points take it: contiguous float32 [K, *W.shape] beside the weights."""
    if ring.dtype != F32 or tuple(ring.shape) != (K, *W.shape) or ring.device != W.device or not ring.is_contiguous():
        raise ValueError(f"an average_update ring must be a contiguous float32 [{K}, {W.shape[0]}, {W.shape[1]}] tensor on {W.device}")
    return _ptr(ring, F32)


def postpre_avg_step(W, s_src, x_src, s_tgt, x_tgt, nu0, nu1, dt, ring_pre, ring_post, idx_pre, idx_post, continuous, squeeze=False,
                     decay=1.0, wmin=None, wmax=None, reduce="sum"):
    """include/snnhip.h f14: one step of MCC PostPre with average_update = ring_pre.shape[0].  idx_*: the ring indices at the start of
    the step; the caller advances the index of every term whose rate is non-zero."""
    B, (Nin, N), K = s_src.shape[0], W.shape, ring_pre.shape[0]
    if _reduce(reduce):             # the reduced update goes into the ring slot; the ring's own mean is unchanged
        check(lib().snn_postpre_avg_step_red(_ptr(W, F32), _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"), _ptr(x_tgt, F32), B, Nin,
                                             N, nu0, nu1, dt, decay, *_bounds(wmin, wmax), int(squeeze), _ring(ring_pre, W, K),
                                             _ring(ring_post, W, K), K, int(continuous), idx_pre, idx_post, _reduce(reduce), _stream()),
              "postpre_avg_step_red")
        return
    check(lib().snn_postpre_avg_step(_ptr(W, F32), _ptr(s_src, "spike"), _ptr(x_src, F32), _ptr(s_tgt, "spike"), _ptr(x_tgt, F32), B, Nin, N,
                                     nu0, nu1, dt, decay, *_bounds(wmin, wmax), int(squeeze), _ring(ring_pre, W, K), _ring(ring_post, W, K),
                                     K, int(continuous), idx_pre, idx_post, _stream()), "postpre_avg_step")


def mstdp_avg_step(W, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, reward, nu0, a_plus, a_minus, decay_plus, decay_minus,
                   ring, idx, continuous, squeeze=False, wdecay=1.0, wmin=None, wmax=None, reward_vec=None, reduce="sum"):
    """include/snnhip.h f14: one step of MCC MSTDP with average_update = ring.shape[0]."""
    B, (Nin, N), K = s_src.shape[0], W.shape, ring.shape[0]
    if _reduce(reduce):
        check(lib().snn_mstdp_avg_step_red(_ptr(W, F32), _ptr(p_plus, F32), _ptr(p_minus, F32), _ptr(s_src_prev, "spike"),
                                           _ptr(s_tgt_prev, "spike"), _ptr(s_src, "spike"), _ptr(s_tgt, "spike"), B, Nin, N, reward,
                                           _ptr(reward_vec, F32, True), nu0, a_plus, a_minus, decay_plus, decay_minus, wdecay,
                                           *_bounds(wmin, wmax), int(squeeze), _ring(ring, W, K), K, int(continuous), idx, _reduce(reduce),
                                           _stream()), "mstdp_avg_step_red")
        return
    check(lib().snn_mstdp_avg_step(_ptr(W, F32), _ptr(p_plus, F32), _ptr(p_minus, F32), _ptr(s_src_prev, "spike"), _ptr(s_tgt_prev, "spike"),
                                   _ptr(s_src, "spike"), _ptr(s_tgt, "spike"), B, Nin, N, reward, _ptr(reward_vec, F32, True), nu0, a_plus,
                                   a_minus, decay_plus, decay_minus, wdecay, *_bounds(wmin, wmax), int(squeeze), _ring(ring, W, K), K,
                                   int(continuous), idx, _stream()), "mstdp_avg_step")


def mstdpet_avg_step(W, e_trace, p_plus, p_minus, s_src_prev, s_tgt_prev, s_src, s_tgt, reward, nu0, dt, a_plus, a_minus, decay_plus,
                     decay_minus, decay_e, tc_e, ring, idx, continuous, wdecay=1.0, wmin=None, wmax=None):
    """include/snnhip.h f14: one step of MCC MSTDPET (batch 1) with average_update = ring.shape[0]."""
    (Nin, N), K = W.shape, ring.shape[0]
    check(lib().snn_mstdpet_avg_step(_ptr(W, F32), _ptr(e_trace, F32), _ptr(p_plus, F32), _ptr(p_minus, F32), _ptr(s_src_prev, "spike"),
                                     _ptr(s_tgt_prev, "spike"), _ptr(s_src, "spike"), _ptr(s_tgt, "spike"), Nin, N, reward, nu0, dt, a_plus,
                                     a_minus, decay_plus, decay_minus, decay_e, tc_e, wdecay, *_bounds(wmin, wmax), _ring(ring, W, K), K,
                                     int(continuous), idx, _stream()), "mstdpet_avg_step")


def normalize(W, norm, use_abs, ws=None):
    Nin, N = W.shape
    if ws is None:
        ws = torch.empty(N, dtype=F32, device=W.device)
    if W.dtype in HALF:
        if use_abs:
            raise NotImplementedError(f"bindsnet_amd: normalisation by absolute column sums computes in float32 only (got {W.dtype})")
        check(lib().snn_normalize_h16(_ptr(W, W.dtype), HALF[W.dtype], Nin, N, norm, _ptr(ws, F32), _stream()), "normalize_h16")
        return
    if isinstance(norm, torch.Tensor):  # one total per target neuron: norm[n] / colsum[n], a true division (snn_normalize_pv)
        check(lib().snn_normalize_pv(_ptr(W, F32), Nin, N, _ptr(norm_vector(norm, N, W.device), F32), int(use_abs), _ptr(ws, F32),
                                     _stream()), "normalize_pv")
        return
    check(lib().snn_normalize(_ptr(W, F32), Nin, N, norm, int(use_abs), _ptr(ws, F32), _stream()), "normalize")


def norm_vector(norm, N, dev):
    """A tensor `norm` as snn_normalize_pv reads it: float32 [N] on `dev` (the tensor itself where it already is; a copy kept on
    it otherwise).  The device takes [N] and [1, N]; the host path runs the reference's expression for every shape."""
    from .learning._descriptor import device_const
    if norm.numel() != N or norm.dim() > 2 or (norm.dim() == 2 and norm.shape[0] != 1):
        raise NotImplementedError(f"bindsnet_amd: a tensor norm on the device has one entry per target neuron, [{N}] or [1, {N}], "
                                  f"not {list(norm.shape)}")
    return device_const(norm, (N,) if norm.dim() == 1 else (1, N), dev)[0]


def normalize_conv2d(W, norm):
    """Conv2dConnection.normalize (topology.py:824-837): every [KH*KW] filter of W [Cout, Cin, KH, KW] scaled to sum `norm`."""
    Cout, Cin, KH, KW = W.shape
    check(lib().snn_normalize_conv2d(_ptr(W, F32), Cout * Cin, KH * KW, float(norm), _stream()), "normalize_conv2d")


def rng_fill_exponential(rng_state, crossings, qbuf, cursor):
    """Device generator: draws for the rows of `crossings` [B,N] that have a non-zero entry."""
    B = crossings.shape[0]
    N = crossings.numel() // B
    check(lib().snn_rng_fill_exponential(_ptr(rng_state, torch.int32), _ptr(crossings, "spike"), B, N, _ptr(qbuf, F32),
                                         _ptr(cursor, torch.int64), _stream()), "rng_fill_exponential")


def encode_bernoulli(datum_flat, steps, max_prob, device):
    """encodings.bernoulli on the device, drawing from the HOST generator's stream (left advanced by steps * n outputs,
    exactly as torch.bernoulli on the CPU would leave it).  datum_flat: 1-D float tensor on any device."""
    from .rng import DeviceGenerator
    x = datum_flat.to(device=device, dtype=F32).contiguous()
    n = x.numel()
    out = torch.empty(steps * n, dtype=torch.uint8, device=x.device)
    with DeviceGenerator(x.device, 1) as g:
        check(lib().snn_encode_bernoulli(_ptr(g.state, torch.int32), _ptr(x, F32), n, steps, float(max_prob), _ptr(out, torch.uint8),
                                         _stream()), "encode_bernoulli")
        g.finish()
    return out


def encode_poisson(datum_flat, steps, dt, seed, device):
    """encodings.poisson_device: Poisson spike trains from a Philox stream keyed by (seed, element)."""
    x = datum_flat.to(device=device, dtype=F32).contiguous()
    n = x.numel()
    out = torch.empty(steps * n, dtype=torch.uint8, device=x.device)
    check(lib().snn_encode_poisson(_ptr(x, F32), n, steps, float(dt), C.c_ulonglong(seed & ((1 << 64) - 1)), _ptr(out, torch.uint8),
                                   _stream()), "encode_poisson")
    return out
