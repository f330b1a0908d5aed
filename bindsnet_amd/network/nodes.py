"""Neuron groups: API mirror of bindsnet/network/nodes.py for the layer types on the hot path
(`Nodes`, `Input`, `McCullochPitts`, `IFNodes`, `LIFNodes`, `BoostedLIFNodes`, `CurrentLIFNodes`, `AdaptiveLIFNodes`,
`DiehlAndCookNodes`, `IzhikevichNodes`, `SRM0Nodes`, `CSRMNodes`); the arithmetic lives in libsnnhip (snn_input_step / snn_lif_step / snn_dc_step /
snn_mcp_step / snn_if_step / snn_boosted_step / snn_clif_step / snn_izh_step / snn_srm0_step / snn_csrm_step).  Each class fills its own snn_layer_desc
(`_describe`), so Network._build_descriptors needs no table of layer types.

State is held in the same attributes as the reference (`s`, `x`, `v`, `refrac_count`, `theta`,
`decay`, `trace_decay`, ...), so monitors, pickling and user code that pokes at them keep working.
"""
from functools import reduce
from operator import mul
from typing import Iterable, Optional, Union

import torch

from .. import _lib, ops

Scalar = Union[float, torch.Tensor]
_SCALARS = None          # collector of the parameter tensors read while run descriptors are being built


def _f(t) -> float:
    """Python float of a 0-dim parameter.  A tensor with more than one element raises: the per-neuron quantities the step kernels
    index by neuron go through Nodes._sv / Nodes._vec instead; everything else (`rest`, `reset`, `refrac`, `lbound`, and
    `trace_scale` without additive traces) fails in the reference too, whose fill_ / masked_fill_ take a 0-dim value only."""
    if isinstance(t, torch.Tensor):
        # .item() on a device tensor is a blocking copy (~15 us each, ~20 per run()): remember the value on the
        # tensor object itself, keyed by its in-place version counter
        if _SCALARS is not None:
            _SCALARS.append((t, t._version))       # (Network._build_descriptors: what the descriptors were filled from)
        hit = getattr(t, "_snn_scalar", None)
        if hit is not None and hit[0] == t._version:
            return hit[1]
        if t.numel() != 1:
            raise NotImplementedError("bindsnet_amd: tensor-valued per-neuron parameters are not supported")
        val = float(t.reshape(()).item())
        try:
            t._snn_scalar = (t._version, val)
        except AttributeError:
            pass
        return val
    return float(t)


def _buf(value, dtype=None) -> torch.Tensor:
    """torch.tensor(value, dtype=...) as the reference writes it (nodes.py:459-472) -- for a tensor-valued parameter that is a detached copy,
    which torch.tensor() makes too but with a UserWarning into every user's log."""
    if isinstance(value, torch.Tensor):
        out = value.detach().clone()
        return out if dtype is None else out.to(dtype)
    return torch.tensor(value) if dtype is None else torch.tensor(value, dtype=dtype)


class Nodes(_lib.TouchingModule, torch.nn.Module):
    """Base class (reference: nodes.py:9-162): spikes `s`, optional trace `x`."""

    def __init__(self, n: Optional[int] = None, shape: Optional[Iterable[int]] = None, traces: bool = False,
                 traces_additive: bool = False, tc_trace: Scalar = 20.0, trace_scale: Scalar = 1.0,
                 sum_input: bool = False, learning: bool = True, **kwargs) -> None:
        super().__init__()
        if n is None and shape is None:
            raise AssertionError("Must provide either no. of neurons or shape of layer")
        self.n = reduce(mul, shape) if n is None else n
        self.shape = [self.n] if shape is None else shape
        assert self.n == reduce(mul, self.shape), "No. of neurons and shape do not match"
        if sum_input and not self._SUMS_INPUT:
            raise NotImplementedError("bindsnet_amd: sum_input=True is outside the accelerated path (only "
                                      "bindsnet.conversion.SubtractiveResetIFNodes takes it)")
        self.traces, self.traces_additive, self.sum_input = traces, traces_additive, sum_input
        self.register_buffer("s", torch.ByteTensor())
        if traces:
            self.register_buffer("x", torch.Tensor())
            self.register_buffer("tc_trace", _buf(tc_trace))
            self.register_buffer("trace_scale", _buf(trace_scale))
            self.register_buffer("trace_decay", torch.empty_like(self.tc_trace))
        if sum_input:
            self.register_buffer("summed", torch.FloatTensor())      # (behind the trace buffers, as in the reference: nodes.py:80-81)
        self.dt = None
        self.batch_size = None
        self.learning = learning

    # -- lifecycle hooks called by Network.add_layer (network.py:130-132) ----------------------
    def compute_decays(self, dt) -> None:
        self.dt = torch.tensor(dt)
        if self.traces:  # same torch op as the reference so the constant is the same float
            self.trace_decay = torch.exp(-self.dt / self.tc_trace.cpu()).to(self.tc_trace.device)

    def set_batch_size(self, batch_size) -> None:
        self.batch_size = batch_size
        dev = self.s.device
        self.s = torch.zeros(batch_size, *self.shape, device=dev, dtype=torch.bool)
        if self.traces:
            self.x = torch.zeros(batch_size, *self.shape, device=dev)
        if self.sum_input:
            self.summed = torch.zeros(batch_size, *self.shape, device=self.summed.device)

    def reset_state_variables(self) -> None:
        self.s.zero_()
        if self.traces:
            self.x.zero_()
        if self.sum_input:
            self.summed.zero_()

    def train(self, mode: bool = True) -> "Nodes":
        self.learning = mode
        return super().train(mode)

    # -- per-neuron parameters --------------------------------------------------------------------
    # The quantities (named after the derived buffers the kernels read: _lib.PERVEC) this class may hold as a tensor with one
    # value per neuron -- the pairs the reference itself runs (INTEGRATION.md section 3 has the table).  `trace_scale` only with
    # additive traces.  The tc_* constants reach the kernels through compute_decays(), as in the reference.
    _PERVEC = ("trace_decay", "trace_scale")
    # whether the class takes sum_input=True (nodes.py:105-107: `summed += x` behind every step); every class without it raises
    _SUMS_INPUT = False

    _SCALAR_ONLY = ()                  # parameters the class refuses as tensors on the device, by name

    def _scalars_only(self) -> None:
        for name in self._SCALAR_ONLY:
            t = getattr(self, name)
            if isinstance(t, torch.Tensor) and t.numel() != 1:
                raise NotImplementedError(f"bindsnet_amd: a tensor-valued `{name}` on {type(self).__name__} is not supported on the device")

    def _state_device(self) -> torch.device:
        v = getattr(self, "v", None)
        return v.device if isinstance(v, torch.Tensor) else self.x.device

    def _vec(self, name: str) -> Optional[torch.Tensor]:
        """Parameter `name` as the step kernels index it by neuron: a contiguous f32 [n] tensor beside the state, or None for a
        scalar (a one-element tensor is a scalar).  A tensor that is not already such a vector is brought over once and kept,
        keyed by its in-place version, like the transposed lateral matrix of IzhikevichNodes."""
        t = getattr(self, name)
        if not isinstance(t, torch.Tensor) or t.numel() == 1:
            return None
        if name not in self._PERVEC or (name == "trace_scale" and not self.traces_additive):
            raise NotImplementedError(f"bindsnet_amd: a tensor-valued per-neuron `{name}` on {type(self).__name__} is not supported"
                                      + (" without additive traces" if name == "trace_scale" and name in self._PERVEC else ""))
        if tuple(t.shape) != tuple(self.shape):
            raise ValueError(f"{type(self).__name__}.{name} has shape {list(t.shape)}, the layer {list(self.shape)}")
        if _SCALARS is not None:
            _SCALARS.append((t, t._version))              # (an in-place change rebuilds the descriptors: the vector may be a copy)
        dev = self._state_device()
        if t.device == dev and t.dtype == torch.float32 and t.is_contiguous():
            return t
        cache = self.__dict__.setdefault("_pervec_dev", {})
        hit = cache.get(name)
        if hit is None or hit[0] is not t or hit[1] != t._version or hit[2].device != dev:
            hit = cache[name] = (t, t._version, t.detach().to(dev, torch.float32).contiguous())
        return hit[2]

    def _sv(self, name: str, pv: dict) -> float:
        """The scalar field for parameter `name`; where it is a per-neuron tensor the vector goes into `pv` and the field is 0."""
        vec = self._vec(name)
        if vec is None:
            return _f(getattr(self, name))
        pv[name] = vec
        return 0.0

    def _pervec_names(self) -> list:
        """Names of this layer's parameters that hold more than one element."""
        names = ("thresh", "rest", "reset", "refrac", "lbound", "tc_decay", "decay", "tc_trace", "trace_decay", "trace_scale",
                 "tc_theta_decay", "theta_decay", "theta_plus", "tc_i_decay", "i_decay")
        return [k for k in names if isinstance(getattr(self, k, None), torch.Tensor) and getattr(self, k).numel() > 1]

    @staticmethod
    def _fill_pv(d: _lib.LayerDesc, pv: dict, keep: list) -> None:
        if pv:
            d.pv = _lib.pervec(pv)
            keep.extend(pv.values())

    # -- descriptor pieces for the run driver ---------------------------------------------------
    def _trace_fields(self, p: _lib.LifParams, pv: Optional[dict] = None) -> None:
        p.traces = int(self.traces)
        if self.traces:
            pv = {} if pv is None else pv
            p.trace_decay, p.trace_scale = self._sv("trace_decay", pv), self._sv("trace_scale", pv)
            p.traces_additive = int(self.traces_additive)

    # float32 [B, n] state tensors (beside `s` and `x`) whose addresses the layer's snn_layer_desc holds
    _STATE = ("v", "refrac_count")
    # float32 tensors the generic plan's step kernels update in place and that a Monitor may record beside `s` and `v`: Network.run
    # copies them out at the end of every timestep (snn_run_desc.records).  `x` joins them on a layer with traces=True.
    _RECORD = ("refrac_count",)

    def _recordable(self) -> tuple:
        return self._RECORD + (("x",) if self.traces else ())

    # device tensors beyond _STATE, `x` and `s` whose addresses the snn_layer_desc holds: watched by the descriptor cache for a re-homed tensor
    _WATCHED = ()

    def _watched(self) -> list:
        return [a for a in self._STATE + ("x",) + self._WATCHED if isinstance(getattr(self, a, None), torch.Tensor)]

    # -- what a layer says about a run before it starts (network/_preflight.py) -------------------
    _gathers_window = False            # whether its input is a window of currents (Connection.compute_window): CSRMNodes

    def _refusals(self, name: str, req):
        """Why the run `req` must not start with this layer, filed as `name`, in it: exceptions (None: nothing)."""
        return ()

    def _multi_device_refusal(self, mode: str, name: str):
        """The layer's reason against parallel.py's mode `mode`, or None."""

    # State tensors Network.reset_state_variables' one launch fills (`v` with `rest`, the rest with zeros), named in the class's OWN body; None: its own reset.
    _RESET_FILL = None

    def _reset_fill(self):                                 # [(tensor, 32-bit pattern)] of `_RESET_FILL`, or None
        names = vars(type(self)).get("_RESET_FILL")
        if names is None:
            return None
        import struct
        return [(getattr(self, a), struct.unpack("<I", struct.pack("<f", _f(self.rest)))[0] if a == "v" else 0)
                for a in names if a != "x" or self.traces]

    def _node_params(self, pv: Optional[dict] = None, **fields) -> _lib.LifParams:
        """snn_lif_params of a layer that has `thresh`: thresh, dt, lbound and the trace fields, plus the named ones.  Per-neuron
        vectors go into `pv` (their scalar fields are then 0)."""
        p, pv = _lib.LifParams(), ({} if pv is None else pv)
        p.thresh, p.dt = self._sv("thresh", pv), _f(self.dt)
        for key, value in fields.items():
            setattr(p, key, self._sv(key, pv) if key in _lib.PERVEC else _f(value))
        lbound = getattr(self, "lbound", None)
        p.has_lbound = int(lbound is not None)
        p.lbound = _f(lbound) if lbound is not None else 0.0
        self._trace_fields(p, pv)
        return p

    def _describe(self, d: _lib.LayerDesc, keep: list, scalars: list) -> int:
        """Fill the class-specific part of this layer's snn_layer_desc `d` (kind, parameters, extra state); the caller has set n,
        v, s, x, refrac, current and the run() options.  `keep` takes tensors that must outlive the launch, `scalars` (tensor,
        version) pairs whose in-place change must rebuild the descriptors.  Returns the number of one_spike draws one step of
        the layer may consume."""
        raise NotImplementedError(f"bindsnet_amd: layer type {type(self).__name__} is outside the accelerated path (Input, "
                                  "McCullochPitts, IFNodes, LIFNodes, BoostedLIFNodes, CurrentLIFNodes, AdaptiveLIFNodes, "
                                  "DiehlAndCookNodes, IzhikevichNodes, SRM0Nodes, CSRMNodes, SubtractiveResetIFNodes, PassThroughNodes)")

    def _host_step(self, x: torch.Tensor) -> None:
        """One step on the host path (network/host_path.py)."""
        raise NotImplementedError(f"bindsnet_amd host path: layer type {type(self).__name__}")

    def _own_spikes(self) -> None:
        """`s` as the step kernels write it: a bool [B, *shape] tensor beside `v`."""
        if self.s.dtype != torch.bool or self.s.shape != self.v.shape:
            self.s = torch.zeros_like(self.v, dtype=torch.bool)

    def forward(self, x: torch.Tensor) -> None:
        raise NotImplementedError


class AbstractInput:
    pass


class Input(Nodes, AbstractInput):
    """User-driven spikes (reference: nodes.py:172-228): `s` aliases the input, trace optional."""
    _RECORD = ()
    _RESET_FILL = ("s", "x")

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)

    def _host_step(self, x: torch.Tensor) -> None:
        from . import host_path
        host_path._step_input(self, x)

    def forward(self, x: torch.Tensor) -> None:
        if not x.is_cuda:                                 # a layer on the host: plain PyTorch (network/host_path.py)
            return self._host_step(x)
        self.s = x
        if self.traces:
            pv = {}
            if x.dtype == torch.float32:                  # a real-valued (analog) input: the trace reads the values themselves
                ops.input_step_real(x.contiguous(), self.x, self._sv("trace_decay", pv), self._sv("trace_scale", pv),
                                    self.traces_additive, pv=pv)
                return
            ops.input_step(x.contiguous(), self.x, self._sv("trace_decay", pv), self._sv("trace_scale", pv), self.traces_additive,
                           pv=pv)


class LIFNodes(Nodes):
    """Leaky integrate-and-fire layer (reference: nodes.py:418-559)."""
    _PERVEC = Nodes._PERVEC + ("thresh", "decay")
    _RESET_FILL = ("s", "x", "refrac_count", "v")

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, thresh: Scalar = -52.0, rest: Scalar = -65.0, reset: Scalar = -65.0,
                 refrac: Union[int, torch.Tensor] = 5, tc_decay: Scalar = 100.0, lbound: float = None,
                 **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)
        self.register_buffer("rest", _buf(rest, torch.float))
        self.register_buffer("reset", _buf(reset, torch.float))
        self.register_buffer("thresh", _buf(thresh, torch.float))
        self.register_buffer("refrac", _buf(refrac))
        self.register_buffer("tc_decay", _buf(tc_decay, torch.float))
        self.register_buffer("decay", torch.zeros(*self.shape))
        self.register_buffer("v", torch.FloatTensor())
        self.register_buffer("refrac_count", torch.FloatTensor())
        self.lbound = None if lbound is None else torch.tensor(lbound, dtype=torch.float)

    def compute_decays(self, dt) -> None:
        super().compute_decays(dt=dt)
        self.decay = torch.exp(-self.dt / self.tc_decay.cpu()).to(self.tc_decay.device)

    def set_batch_size(self, batch_size) -> None:
        super().set_batch_size(batch_size=batch_size)
        dev = self.v.device
        self.v = self.rest.to(dev) * torch.ones(batch_size, *self.shape, device=dev)
        self.refrac_count = torch.zeros_like(self.v)

    def reset_state_variables(self) -> None:
        super().reset_state_variables()
        self.v.fill_(_f(self.rest))
        self.refrac_count.zero_()

    def _lif_params(self, pv: Optional[dict] = None) -> _lib.LifParams:
        """snn_lif_params; per-neuron vectors go into `pv` (the callers hand pv["thresh"] on through the older thresh_vec field)."""
        pv = {} if pv is None else pv
        p = _lib.LifParams()
        p.decay, p.rest, p.reset = self._sv("decay", pv), _f(self.rest), _f(self.reset)
        p.thresh = self._sv("thresh", pv)
        p.refrac, p.dt = _f(self.refrac), _f(self.dt)
        p.has_lbound = int(self.lbound is not None)
        p.lbound = _f(self.lbound) if self.lbound is not None else 0.0
        self._trace_fields(p, pv)
        return p

    def _describe(self, d, keep, scalars) -> int:
        d.kind = _lib.LAYER_LIF
        pv = {}
        d.p.lif = self._lif_params(pv)
        tv = pv.pop("thresh", None)                       # per-neuron thresholds (nodes.py:425-498; generic plan)
        self._fill_pv(d, pv, keep)
        if tv is not None:
            keep.append(tv)
            d.thresh_vec = _lib.dptr(tv)
        return 0

    def _host_step(self, x: torch.Tensor) -> None:
        from . import host_path
        host_path._step_lif(self, x)

    def forward(self, x: torch.Tensor) -> None:
        """One step (nodes.py:500-529); `x` is masked in place where refractory, as in the reference."""
        if not self.v.is_cuda:                            # a layer on the host: plain PyTorch (network/host_path.py)
            return self._host_step(x)
        if self.s.dtype != torch.bool or self.s.shape != self.v.shape:
            self.s = torch.zeros_like(self.v, dtype=torch.bool)
        pv = {}
        p = self._lif_params(pv)
        ops.lif_step(self.v, self.refrac_count, self.s, self.x if self.traces else None, x, p, thresh_vec=pv.pop("thresh", None), pv=pv)


class _AdaptiveThresholdNodes(Nodes):
    """What DiehlAndCookNodes (nodes.py:981-1144) and AdaptiveLIFNodes (nodes.py:829-978) share: the same buffers, decays and
    membrane / threshold arithmetic (SNN_LAYER_DC).  They differ only in DiehlAndCookNodes' one-spike arbitration.  Private, so
    that neither class is an instance of the other, as in the reference."""
    _PERVEC = Nodes._PERVEC + ("thresh", "decay", "theta_decay", "theta_plus")
    _RECORD = ("refrac_count", "theta")
    _WATCHED = ("theta",)

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, thresh: Scalar = -52.0, rest: Scalar = -65.0, reset: Scalar = -65.0,
                 refrac: Union[int, torch.Tensor] = 5, tc_decay: Scalar = 100.0, theta_plus: Scalar = 0.05,
                 tc_theta_decay: Scalar = 1e7, lbound: float = None, one_spike: bool = True, **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)
        self.register_buffer("rest", _buf(rest))
        self.register_buffer("reset", _buf(reset))
        self.register_buffer("thresh", _buf(thresh))
        self.register_buffer("refrac", _buf(refrac))
        self.register_buffer("tc_decay", _buf(tc_decay))
        self.register_buffer("decay", torch.empty_like(self.tc_decay, dtype=torch.float32))
        self.register_buffer("theta_plus", _buf(theta_plus))
        self.register_buffer("tc_theta_decay", _buf(tc_theta_decay))
        self.register_buffer("theta_decay", torch.empty_like(self.tc_theta_decay))
        self.register_buffer("v", torch.FloatTensor())
        self.register_buffer("theta", torch.zeros(*self.shape))
        self.register_buffer("refrac_count", torch.FloatTensor())
        self.lbound = lbound
        self.one_spike = one_spike

    def compute_decays(self, dt) -> None:
        super().compute_decays(dt=dt)
        dev = self.tc_decay.device
        self.decay = torch.exp(-self.dt / self.tc_decay.cpu()).to(dev)
        self.theta_decay = torch.exp(-self.dt / self.tc_theta_decay.cpu()).to(dev)

    def set_batch_size(self, batch_size) -> None:
        super().set_batch_size(batch_size=batch_size)
        dev = self.v.device
        self.v = self.rest.to(dev) * torch.ones(batch_size, *self.shape, device=dev)
        self.refrac_count = torch.zeros_like(self.v)

    def reset_state_variables(self) -> None:  # theta is NOT reset (nodes.py:1113-1120)
        super().reset_state_variables()
        self.v.fill_(_f(self.rest))
        self.refrac_count.zero_()

    def _dc_params(self, pv: Optional[dict] = None) -> _lib.DcParams:
        """snn_dc_params; per-neuron vectors go into `pv`."""
        pv = {} if pv is None else pv
        p = _lib.DcParams()
        l = p.lif
        l.decay, l.rest, l.reset, l.thresh = self._sv("decay", pv), _f(self.rest), _f(self.reset), self._sv("thresh", pv)
        l.refrac, l.dt = _f(self.refrac), _f(self.dt)
        l.has_lbound = int(self.lbound is not None)
        l.lbound = (_f(self.lbound) if isinstance(self.lbound, torch.Tensor) else float(self.lbound)) if self.lbound is not None else 0.0
        self._trace_fields(l, pv)
        p.theta_decay, p.theta_plus = self._sv("theta_decay", pv), self._sv("theta_plus", pv)
        p.learning, p.one_spike = int(self.learning), int(self.one_spike)
        return p

    def _describe(self, d, keep, scalars) -> int:
        pv = {}
        d.kind, d.p, d.theta = _lib.LAYER_DC, self._dc_params(pv), _lib.dptr(self.theta)
        self._fill_pv(d, pv, keep)
        return self.v.shape[0] * self.n if self.one_spike else 0

    def _host_step(self, x: torch.Tensor) -> None:
        from . import host_path
        host_path._step_dc(self, x)

    def forward(self, x: torch.Tensor) -> None:
        """One step (nodes.py:1069-1111).  The winner draw consumes the global CPU generator
        exactly like torch.multinomial does in the reference (see bindsnet_amd/rng.py)."""
        if not self.v.is_cuda:                            # a layer on the host: plain PyTorch (network/host_path.py)
            return self._host_step(x)
        from ..rng import NoiseStream
        if self.s.dtype != torch.bool or self.s.shape != self.v.shape:
            self.s = torch.zeros_like(self.v, dtype=torch.bool)
        B = self.v.shape[0]
        pv = {}
        p = self._dc_params(pv)                            # (before the draws: a refused parameter leaves the generator alone)
        with NoiseStream(self.v.device, max_draws=B * self.n if self.one_spike else 0) as ns:
            ops.dc_step(self.v, self.refrac_count, self.s, self.x if self.traces else None, self.theta, x,
                        p, ns.q, ns.cursor, ns.status, pv=pv)


class DiehlAndCookNodes(_AdaptiveThresholdNodes):
    """LIF with adaptive threshold and one-spike arbitration (reference: nodes.py:981-1144)."""
    _RESET_FILL = LIFNodes._RESET_FILL

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, thresh: Scalar = -52.0, rest: Scalar = -65.0, reset: Scalar = -65.0,
                 refrac: Union[int, torch.Tensor] = 5, tc_decay: Scalar = 100.0, theta_plus: Scalar = 0.05,
                 tc_theta_decay: Scalar = 1e7, lbound: float = None, one_spike: bool = True, **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input, thresh=thresh, rest=rest, reset=reset, refrac=refrac,
                         tc_decay=tc_decay, theta_plus=theta_plus, tc_theta_decay=tc_theta_decay, lbound=lbound,
                         one_spike=one_spike)


class AdaptiveLIFNodes(_AdaptiveThresholdNodes):
    """LIF with an adaptive threshold (reference: nodes.py:829-978): DiehlAndCookNodes' step without the one-spike
    arbitration -- every neuron that crosses its threshold spikes.  Same constructor arguments, buffers and decays as the
    reference; runs as an SNN_LAYER_DC layer with one_spike = 0."""
    _RESET_FILL = LIFNodes._RESET_FILL

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, rest: Scalar = -65.0, reset: Scalar = -65.0, thresh: Scalar = -52.0,
                 refrac: Union[int, torch.Tensor] = 5, tc_decay: Scalar = 100.0, theta_plus: Scalar = 0.05,
                 tc_theta_decay: Scalar = 1e7, lbound: float = None, **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input, thresh=thresh, rest=rest, reset=reset, refrac=refrac,
                         tc_decay=tc_decay, theta_plus=theta_plus, tc_theta_decay=tc_theta_decay, lbound=lbound,
                         one_spike=False)


class McCullochPitts(Nodes):
    """McCulloch-Pitts layer (reference: nodes.py:231-305): v = x, s = v >= thresh.  The reference makes `v` an alias of the
    input tensor; on the device this layer holds its own [B, n] copy of it (the step kernel writes it), on the host it
    aliases like the reference."""
    _STATE = ("v",)
    _RECORD = ()
    _PERVEC = Nodes._PERVEC + ("thresh",)

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, thresh: Scalar = 1.0, **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)
        self.register_buffer("thresh", _buf(thresh, torch.float))
        self.register_buffer("v", torch.FloatTensor())

    def set_batch_size(self, batch_size) -> None:
        super().set_batch_size(batch_size=batch_size)
        self.v = torch.zeros(batch_size, *self.shape, device=self.v.device)

    def _describe(self, d, keep, scalars) -> int:
        pv = {}
        d.kind, d.p.lif = _lib.LAYER_MCP, self._node_params(pv)
        self._fill_pv(d, pv, keep)
        return 0

    def _host_step(self, x: torch.Tensor) -> None:
        from . import host_path
        host_path._step_mcp(self, x)

    def forward(self, x: torch.Tensor) -> None:
        """One step (nodes.py:278-288)."""
        if not x.is_cuda:
            return self._host_step(x)
        self._own_spikes()
        pv = {}
        p = self._node_params(pv)
        ops.mcp_step(self.v, self.s, self.x if self.traces else None, x, p, pv=pv)


class IFNodes(Nodes):
    """Integrate-and-fire layer (reference: nodes.py:308-415): no decay, no rest; state starts at `reset`."""
    _PERVEC = Nodes._PERVEC + ("thresh",)

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, thresh: Scalar = -52.0, reset: Scalar = -65.0, refrac: Union[int, torch.Tensor] = 5,
                 lbound: float = None, **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)
        self.register_buffer("reset", _buf(reset, torch.float))
        self.register_buffer("thresh", _buf(thresh, torch.float))
        self.register_buffer("refrac", _buf(refrac))
        self.register_buffer("v", torch.FloatTensor())
        self.register_buffer("refrac_count", torch.FloatTensor())
        self.lbound = lbound

    def set_batch_size(self, batch_size) -> None:
        super().set_batch_size(batch_size=batch_size)
        dev = self.v.device
        self.v = self.reset.to(dev) * torch.ones(batch_size, *self.shape, device=dev)
        self.refrac_count = torch.zeros_like(self.v)

    def reset_state_variables(self) -> None:
        super().reset_state_variables()
        self.v.fill_(_f(self.reset))
        self.refrac_count.zero_()

    def _params(self, pv: Optional[dict] = None) -> _lib.LifParams:
        return self._node_params(pv, reset=self.reset, refrac=self.refrac)

    def _describe(self, d, keep, scalars) -> int:
        pv = {}
        d.kind, d.p.lif = _lib.LAYER_IF, self._params(pv)
        self._fill_pv(d, pv, keep)
        return 0

    def _host_step(self, x: torch.Tensor) -> None:
        from . import host_path
        host_path._step_if(self, x)

    def forward(self, x: torch.Tensor) -> None:
        """One step (nodes.py:371-395)."""
        if not self.v.is_cuda:
            return self._host_step(x)
        self._own_spikes()
        pv = {}
        p = self._params(pv)
        ops.if_step(self.v, self.refrac_count, self.s, self.x if self.traces else None, x, p, pv=pv)


class BoostedLIFNodes(Nodes):
    """LIF without rest, reset value or lower bound (reference: nodes.py:562-678): the membrane decays towards 0 and is reset
    to 0.  `refrac_count` is an integer scalar until set_batch_size() makes it a float [B, n] tensor, as in the reference."""
    _PERVEC = Nodes._PERVEC + ("thresh", "decay")

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, thresh: Scalar = 13.0, refrac: Union[int, torch.Tensor] = 5, tc_decay: Scalar = 100.0,
                 **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)
        self.register_buffer("thresh", _buf(thresh, torch.float))
        self.register_buffer("refrac", _buf(refrac))
        self.register_buffer("tc_decay", _buf(tc_decay, torch.float))
        self.register_buffer("decay", torch.zeros(*self.shape))
        self.register_buffer("v", torch.FloatTensor())
        self.register_buffer("refrac_count", torch.tensor(0))

    def compute_decays(self, dt) -> None:
        super().compute_decays(dt=dt)
        self.decay = torch.exp(-self.dt / self.tc_decay.cpu()).to(self.tc_decay.device)

    def set_batch_size(self, batch_size) -> None:
        super().set_batch_size(batch_size=batch_size)
        self.v = torch.zeros(batch_size, *self.shape, device=self.v.device)
        self.refrac_count = torch.zeros_like(self.v, device=self.refrac_count.device)

    def reset_state_variables(self) -> None:
        super().reset_state_variables()
        self.v.fill_(0)
        self.refrac_count.zero_()

    def _params(self, pv: Optional[dict] = None) -> _lib.LifParams:
        return self._node_params(pv, decay=self.decay, refrac=self.refrac)

    def _describe(self, d, keep, scalars) -> int:
        pv = {}
        d.kind, d.p.lif = _lib.LAYER_BOOSTED, self._params(pv)
        self._fill_pv(d, pv, keep)
        return 0

    def _host_step(self, x: torch.Tensor) -> None:
        from . import host_path
        host_path._step_boosted(self, x)

    def forward(self, x: torch.Tensor) -> None:
        """One step (nodes.py:621-648); `x` is masked in place where refractory, as in the reference."""
        if not self.v.is_cuda:
            return self._host_step(x)
        self._own_spikes()
        pv = {}
        p = self._params(pv)
        ops.boosted_step(self.v, self.refrac_count, self.s, self.x if self.traces else None, x, p, pv=pv)


class CurrentLIFNodes(Nodes):
    """Current-based LIF layer (reference: nodes.py:681-826): the input feeds a decaying synaptic current `i`, which feeds
    the membrane."""
    _STATE = ("v", "refrac_count", "i")
    _RECORD = ("refrac_count", "i")
    _PERVEC = Nodes._PERVEC + ("thresh", "decay", "i_decay")

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, thresh: Scalar = -52.0, rest: Scalar = -65.0, reset: Scalar = -65.0,
                 refrac: Union[int, torch.Tensor] = 5, tc_decay: Scalar = 100.0, tc_i_decay: Scalar = 2.0,
                 lbound: float = None, **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)
        self.register_buffer("rest", _buf(rest))
        self.register_buffer("reset", _buf(reset))
        self.register_buffer("thresh", _buf(thresh))
        self.register_buffer("refrac", _buf(refrac))
        self.register_buffer("tc_decay", _buf(tc_decay))
        self.register_buffer("decay", torch.empty_like(self.tc_decay))
        self.register_buffer("tc_i_decay", _buf(tc_i_decay))
        self.register_buffer("i_decay", torch.empty_like(self.tc_i_decay))
        self.register_buffer("v", torch.FloatTensor())
        self.register_buffer("i", torch.FloatTensor())
        self.register_buffer("refrac_count", torch.FloatTensor())
        self.lbound = lbound

    def compute_decays(self, dt) -> None:
        super().compute_decays(dt=dt)
        dev = self.tc_decay.device
        self.decay = torch.exp(-self.dt / self.tc_decay.cpu()).to(dev)
        self.i_decay = torch.exp(-self.dt / self.tc_i_decay.cpu()).to(dev)

    def set_batch_size(self, batch_size) -> None:
        super().set_batch_size(batch_size=batch_size)
        dev = self.v.device
        self.v = self.rest.to(dev) * torch.ones(batch_size, *self.shape, device=dev)
        self.i = torch.zeros_like(self.v, device=self.i.device)
        self.refrac_count = torch.zeros_like(self.v, device=self.refrac_count.device)

    def reset_state_variables(self) -> None:
        super().reset_state_variables()
        self.v.fill_(_f(self.rest))
        self.i.zero_()
        self.refrac_count.zero_()

    def _params(self, pv: Optional[dict] = None) -> _lib.LifParams:
        return self._node_params(pv, decay=self.decay, rest=self.rest, reset=self.reset, refrac=self.refrac)

    def _describe(self, d, keep, scalars) -> int:
        pv = {}
        d.kind, d.p.lif = _lib.LAYER_CURRENT, self._params(pv)
        d.aux, d.aux_decay = _lib.dptr(self.i), self._sv("i_decay", pv)
        self._fill_pv(d, pv, keep)
        return 0

    def _host_step(self, x: torch.Tensor) -> None:
        from . import host_path
        host_path._step_clif(self, x)

    def forward(self, x: torch.Tensor) -> None:
        """One step (nodes.py:762-791)."""
        if not self.v.is_cuda:
            return self._host_step(x)
        self._own_spikes()
        pv = {}
        p, i_decay = self._params(pv), self._sv("i_decay", pv)
        ops.clif_step(self.v, self.refrac_count, self.i, self.s, self.x if self.traces else None, x, p, i_decay, pv=pv)


class IzhikevichNodes(Nodes):
    """Izhikevich layer (reference: nodes.py:1147-1316) with its lateral matrix `S`.  The constructor draws `r` and `S` from
    the global generator in the reference's order and leaves it where the reference does.  `n` is required.

    On the device the step is one kernel (snn_izh_step); it reads the lateral matrix transposed, from a copy kept beside the
    user-visible `S` and refreshed when `S` is replaced, changed in place or moved.  Layers of more than `_lib.IZH_MAX_N`
    neurons raise NotImplementedError there: the lateral sum's order is pinned against torch up to that size only."""
    _STATE = ("v", "u")
    _RECORD = ()
    _WATCHED = ("a", "b", "c", "d")
    _PERVEC = Nodes._PERVEC + ("thresh",)

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, excitatory: float = 1, thresh: Scalar = 45.0, rest: Scalar = -65.0, lbound: float = None,
                 **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)
        if n is None:
            raise TypeError("IzhikevichNodes needs `n` (the reference draws torch.rand(n))")
        self.register_buffer("rest", _buf(rest))
        self.register_buffer("thresh", _buf(thresh))
        self.lbound = lbound
        excitatory = min(1, max(0, excitatory))

        def population(count: int, excit: bool):
            """(r, a, b, c, d, columns of S) of `count` regular-spiking excitatory / fast-spiking inhibitory neurons: r first,
            then S, from the global generator."""
            r = torch.rand(count)
            if excit:
                return (r, 0.02 * torch.ones(count), 0.2 * torch.ones(count), -65.0 + 15 * (r ** 2), 8 - 6 * (r ** 2),
                        0.5 * torch.rand(n, count))
            return r, 0.02 + 0.08 * r, 0.25 - 0.05 * r, -65.0 * torch.ones(count), 2 * torch.ones(count), -torch.rand(n, count)

        if excitatory == 1 or excitatory == 0:
            parts = population(n, excitatory == 1)
            flags = (torch.ones(n) if excitatory == 1 else torch.zeros(n)).byte()
        else:
            ex = int(n * excitatory)
            parts = [torch.zeros(n) for _ in range(5)] + [torch.zeros(n, n)]
            for cols, excit in ((slice(0, ex), True), (slice(ex, n), False)):      # excitatory draws first
                for whole, part in zip(parts, population(len(range(n)[cols]), excit)):
                    whole[..., cols] = part
            flags = torch.zeros(n).byte()
            flags[:ex] = 1
        for name, value in zip(("r", "a", "b", "c", "d", "S"), parts):
            self.register_buffer(name, value)
        self.register_buffer("excitatory", flags)
        self.register_buffer("v", self.rest * torch.ones(n))
        self.register_buffer("u", self.b * self.v)

    def set_batch_size(self, batch_size) -> None:
        super().set_batch_size(batch_size=batch_size)
        dev = self.v.device
        self.v = self.rest.to(dev) * torch.ones(batch_size, *self.shape, device=dev)
        self.u = self.b * self.v

    def reset_state_variables(self) -> None:
        super().reset_state_variables()
        self.v.fill_(_f(self.rest))
        self.u = self.b * self.v

    def _St(self) -> torch.Tensor:
        """The lateral matrix as the step kernel reads it: transposed, contiguous f32 beside `v` (cached like Nodes._vec)."""
        S = self.S
        cached = self.__dict__.get("_St_dev")
        if cached is None or cached[0] is not S or cached[1] != S._version or cached[2].device != self.v.device:
            cached = self.__dict__["_St_dev"] = (S, S._version, S.detach().to(self.v.device, torch.float32).t().contiguous())
        return cached[2]

    def _abcd(self):
        _f(self.rest)       # the step never reads `rest`, reset_state_variables() does: a tensor is refused before the run, not after
        if self.n > _lib.IZH_MAX_N:
            raise NotImplementedError(f"bindsnet_amd: IzhikevichNodes of more than {_lib.IZH_MAX_N} neurons (the order of the "
                                      "lateral sum is pinned against torch up to that size only)")
        out = []
        for name in ("a", "b", "c", "d"):
            t = getattr(self, name)
            if t.device != self.v.device or t.dtype != torch.float32 or t.numel() != self.n or not t.is_contiguous():
                raise ValueError(f"IzhikevichNodes.{name} must be a contiguous float32 [{self.n}] tensor on {self.v.device}")
            out.append(t)
        if tuple(self.S.shape) != (self.n, self.n):
            raise ValueError(f"IzhikevichNodes.S must be [{self.n}, {self.n}]")
        return out

    def _describe(self, d, keep, scalars) -> int:
        a, b, c, dd = self._abcd()
        St = self._St()
        keep.append(St)
        scalars.append((self.S, self.S._version))         # (an in-place change of S rebuilds: St is a copy)
        pv = {}
        d.kind, d.p.lif = _lib.LAYER_IZH, self._node_params(pv)
        self._fill_pv(d, pv, keep)
        d.aux = _lib.dptr(self.u)
        d.izh_a, d.izh_b, d.izh_c, d.izh_d, d.izh_St = (_lib.dptr(t) for t in (a, b, c, dd, St))
        return 0

    def _host_step(self, x: torch.Tensor) -> None:
        from . import host_path
        host_path._step_izh(self, x)

    def forward(self, x: torch.Tensor) -> None:
        """One step (nodes.py:1265-1296); the lateral sum is added to `x` in place, as in the reference."""
        if not self.v.is_cuda:
            return self._host_step(x)
        self._own_spikes()
        a, b, c, d = self._abcd()
        pv = {}
        p = self._node_params(pv)
        ops.izh_step(self.v, self.u, self.s, self.x if self.traces else None, x, a, b, c, d, self._St(), p, pv=pv)


class SRM0Nodes(Nodes):
    """Simplified spike response model neurons with a stochastic threshold -- escape noise (reference: nodes.py:1555-1701).  Each
    step draws one uniform number per neuron and sample from torch's GLOBAL CPU generator (`torch.rand_like(s_prob) < s_prob`);
    on the device the step kernel (snn_srm0_step) consumes that generator's stream in the same positions (rng.DeviceGenerator),
    so the spikes are the reference's.  `rho` and `s_prob` are attributes after a step, as in the reference; on the device the
    kernel writes both (`rho` is taken from the voltage before the reset, so it cannot be recomputed from `v`).  The two
    exponentials are the device's expf, a 1-ulp function like torch's own: `rho` and `s_prob` agree with the reference to a few
    ulp, everything else bit for bit whenever the spikes do."""
    _PERVEC = Nodes._PERVEC + ("thresh", "decay")
    _SCALAR_ONLY = ("eps_0", "rho_0", "d_thresh", "rest", "reset")      # refused as tensors on the device, by name
    _WATCHED = ("s_prob", "rho")

    def _multi_device_refusal(self, mode, name):
        return NotImplementedError(f"{mode}: layer '{name}' (SRM0Nodes) draws from the host generator in the global batch's order, which "
                                   "the multi-device modes do not reproduce; run the network on one device")

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, thresh: Scalar = -50.0, rest: Scalar = -70.0, reset: Scalar = -70.0,
                 refrac: Union[int, torch.Tensor] = 5, tc_decay: Scalar = 10.0, lbound: float = None, eps_0: Scalar = 1.0,
                 rho_0: Scalar = 1.0, d_thresh: Scalar = 5.0, **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)
        self.register_buffer("rest", _buf(rest))
        self.register_buffer("reset", _buf(reset))
        self.register_buffer("thresh", _buf(thresh))
        self.register_buffer("refrac", _buf(refrac))
        self.register_buffer("tc_decay", _buf(tc_decay))
        self.register_buffer("decay", _buf(tc_decay))      # (set in compute_decays, as in the reference)
        self.register_buffer("eps_0", _buf(eps_0))
        self.register_buffer("rho_0", _buf(rho_0))
        self.register_buffer("d_thresh", _buf(d_thresh))
        self.register_buffer("v", torch.FloatTensor())
        self.register_buffer("refrac_count", torch.FloatTensor())
        self.lbound = lbound

    def compute_decays(self, dt) -> None:
        super().compute_decays(dt=dt)
        self.decay = torch.exp(-self.dt / self.tc_decay.cpu()).to(self.tc_decay.device)

    def set_batch_size(self, batch_size) -> None:
        super().set_batch_size(batch_size=batch_size)
        dev = self.v.device
        self.v = self.rest.to(dev) * torch.ones(batch_size, *self.shape, device=dev)
        self.refrac_count = torch.zeros_like(self.v, device=self.refrac_count.device)

    def reset_state_variables(self) -> None:
        super().reset_state_variables()
        self.v.fill_(_f(self.rest))
        self.refrac_count.zero_()

    def _params(self, pv: Optional[dict] = None) -> _lib.LifParams:
        self._scalars_only()
        return self._node_params(pv, decay=self.decay, rest=self.rest, reset=self.reset, refrac=self.refrac)

    def _prob_buffers(self):
        """`s_prob` and `rho` as the step kernel writes them: f32 tensors beside `v`, created on first use (plain attributes, as in
        the reference)."""
        for name in ("s_prob", "rho"):
            t = self.__dict__.get(name)
            if not isinstance(t, torch.Tensor) or t.shape != self.v.shape or t.device != self.v.device or t.dtype != torch.float32 \
                    or not t.is_contiguous():
                setattr(self, name, torch.zeros_like(self.v))
        return self.s_prob, self.rho

    def _describe(self, d, keep, scalars) -> int:
        pv = {}
        d.kind, d.p.lif = _lib.LAYER_SRM0, self._params(pv)
        d.srm_eps0, d.srm_rho0, d.srm_dthresh = _f(self.eps_0), _f(self.rho_0), _f(self.d_thresh)
        s_prob, rho = self._prob_buffers()
        d.srm_sprob, d.srm_rho = _lib.dptr(s_prob), _lib.dptr(rho)
        self._fill_pv(d, pv, keep)
        return 1                                          # (> 0: the run takes the host generator to the device; no Exp(1) draws)

    def _host_step(self, x: torch.Tensor) -> None:
        from . import host_path
        host_path._step_srm0(self, x)

    def forward(self, x: torch.Tensor) -> None:
        """One step (nodes.py:1639-1671); the draw consumes the global CPU generator exactly as torch.rand_like does there."""
        if not self.v.is_cuda:
            return self._host_step(x)
        from ..rng import DeviceGenerator
        self._own_spikes()
        pv = {}
        p = self._params(pv)                              # (before the draws: a refused parameter leaves the generator alone)
        eps_0, rho_0, d_thresh = _f(self.eps_0), _f(self.rho_0), _f(self.d_thresh)
        s_prob, rho = self._prob_buffers()
        with DeviceGenerator(self.v.device, 1) as g:
            ops.srm0_step(g.state, self.v, self.refrac_count, self.s, self.x if self.traces else None, x, s_prob, rho, p,
                          eps_0, rho_0, d_thresh, pv=pv)
            g.finish()


class CSRMNodes(Nodes):
    """Cumulative spike response model neurons (reference: nodes.py:1319-1552).  Unlike every other layer its input is a WINDOW,
    `[B, res_window_size, n]`: the last `res_window_size` spike vectors of its sources, each multiplied by the current weights
    (Connection.compute_window).  A step contracts that window with the response kernel and the layer's own last
    `ref_window_size` spikes (`last_spikes`) with the refractory kernel.  There is no reset and no refractory counter, `theta` is
    shared by the batch, and reset_state_variables() clears neither `last_spikes` nor the connections' windows -- all as in the
    reference.  `resKernel` and `refKernel` are made on the host with the reference's own expressions.

    On the device the step is snn_csrm_step: the two contractions run in ascending slot order, product then add, which is not the
    order of torch's einsum -- `v` agrees with the reference to rounding, everything that depends on `v` only through the spikes
    bit for bit whenever the spikes do."""
    _STATE = ("v",)
    _RECORD = ("theta",)
    _WATCHED = ("theta", "last_spikes", "resKernel", "refKernel")
    _gathers_window = True
    _PERVEC = Nodes._PERVEC + ("thresh", "decay", "theta_decay", "theta_plus")
    # refused as tensors on the device, by name
    _SCALAR_ONLY = ("rest", "tau", "reset_const")

    def __init__(self, n=None, shape=None, traces=False, traces_additive=False, tc_trace=20.0, trace_scale=1.0,
                 sum_input=False, rest: Scalar = -65.0, thresh: Scalar = -52.0, responseKernel: str = "ExponentialKernel",
                 refractoryKernel: str = "EtaKernel", tau: Scalar = 1, res_window_size: Scalar = 20, ref_window_size: Scalar = 10,
                 reset_const: Scalar = 50, tc_decay: Scalar = 100.0, theta_plus: Scalar = 0.05, tc_theta_decay: Scalar = 1e7,
                 lbound: float = None, **kwargs) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)
        self.register_buffer("rest", _buf(rest))
        self.register_buffer("thresh", _buf(thresh))
        self.register_buffer("tau", _buf(tau))
        self.register_buffer("reset_const", _buf(reset_const))
        self.register_buffer("res_window_size", _buf(res_window_size))
        self.register_buffer("ref_window_size", _buf(ref_window_size))
        self.register_buffer("tc_decay", _buf(tc_decay))
        self.register_buffer("decay", torch.empty_like(self.tc_decay, dtype=torch.float32))
        self.register_buffer("theta_plus", _buf(theta_plus))
        self.register_buffer("tc_theta_decay", _buf(tc_theta_decay))
        self.register_buffer("theta_decay", torch.empty_like(self.tc_theta_decay))
        self.register_buffer("v", torch.FloatTensor())
        self.register_buffer("last_spikes", torch.ByteTensor())
        self.register_buffer("theta", torch.zeros(*self.shape))
        self.lbound = lbound
        self.responseKernel = responseKernel
        self.refractoryKernel = refractoryKernel
        self.register_buffer("resKernel", torch.FloatTensor())
        self.register_buffer("refKernel", torch.FloatTensor())

    def compute_decays(self, dt) -> None:
        super().compute_decays(dt=dt)
        dev = self.tc_decay.device
        self.decay = torch.exp(-self.dt / self.tc_decay.cpu()).to(dev)
        self.theta_decay = torch.exp(-self.dt / self.tc_theta_decay.cpu()).to(dev)

    def set_batch_size(self, batch_size) -> None:
        super().set_batch_size(batch_size=batch_size)
        dev = self.v.device
        self.v = self.rest.to(dev) * torch.ones(batch_size, *self.shape, device=dev)
        self.last_spikes = torch.zeros(batch_size, self.ref_window_size.cpu(), *self.shape).to(dev)   # (a float size: TypeError, as there)
        resKernels = {"AlphaKernel": self.AlphaKernel, "AlphaKernelSLAYER": self.AlphaKernelSLAYER, "LaplacianKernel": self.LaplacianKernel,
                      "ExponentialKernel": self.ExponentialKernel, "RectangularKernel": self.RectangularKernel,
                      "TriangularKernel": self.TriangularKernel}
        if self.responseKernel not in resKernels.keys():
            raise Exception(" The given response Kernel is not implemented")
        self.resKernel = resKernels[self.responseKernel](self.dt).to(dev)
        refKernels = {"EtaKernel": self.EtaKernel}
        if self.refractoryKernel not in refKernels.keys():
            raise Exception(" The given refractory Kernel is not implemented")
        self.refKernel = refKernels[self.refractoryKernel](self.dt).to(dev)

    # The kernels, nodes.py:1519-1552: the reference's expressions, evaluated on the host (the last bit of exp belongs to it).
    def AlphaKernel(self, dt):
        tau = self.tau.cpu()
        t = torch.arange(0, self.res_window_size.cpu(), dt)
        kernelVec = (1 / (tau**2)) * t * torch.exp(-t / tau)
        return torch.flip(kernelVec, [0])

    def AlphaKernelSLAYER(self, dt):
        tau = self.tau.cpu()
        t = torch.arange(0, self.res_window_size.cpu(), dt)
        kernelVec = (1 / tau) * t * torch.exp(1 - t / tau)
        return torch.flip(kernelVec, [0])

    def LaplacianKernel(self, dt):
        tau = self.tau.cpu()
        t = torch.arange(0, self.res_window_size.cpu(), dt)
        kernelVec = (1 / (tau * 2)) * torch.exp(-1 * torch.abs(t / tau))
        return torch.flip(kernelVec, [0])

    def ExponentialKernel(self, dt):
        tau = self.tau.cpu()
        t = torch.arange(0, self.res_window_size.cpu(), dt)
        kernelVec = (1 / tau) * torch.exp(-t / tau)
        return torch.flip(kernelVec, [0])

    def RectangularKernel(self, dt):
        tau = self.tau.cpu()
        t = torch.arange(0, self.res_window_size.cpu(), dt)        # noqa: F841 (the reference forgets to use it: the kernel is 0-dim)
        kernelVec = 1 / (tau * 2)
        return torch.flip(kernelVec, [0])

    def TriangularKernel(self, dt):
        tau = self.tau.cpu()
        t = torch.arange(0, self.res_window_size.cpu(), dt)
        kernelVec = (1 / tau) * (1 - (t / tau))
        return torch.flip(kernelVec, [0])

    def EtaKernel(self, dt):
        tau = self.tau.cpu()
        t = torch.arange(0, self.ref_window_size.cpu(), dt)
        kernelVec = -self.reset_const.cpu() * torch.exp(-t / tau)
        return torch.flip(kernelVec, [0])

    def reset_state_variables(self) -> None:      # last_spikes is NOT cleared (nodes.py:1466-1472)
        super().reset_state_variables()
        self.v.fill_(_f(self.rest))

    def _window_sizes(self):
        """(res_window_size, ref_window_size) as ints; a non-integer res_window_size raises the TypeError the reference's
        torch.zeros(batch, res_window_size, ...) raises in the first step."""
        for name in ("res_window_size", "ref_window_size"):
            t = getattr(self, name)
            if t.is_floating_point() or t.numel() != 1:
                raise TypeError(f"zeros(): argument 'size' must be tuple of ints, but CSRMNodes.{name} is {t.dtype} with {t.numel()} element(s)")
        return int(self.res_window_size), int(self.ref_window_size)

    def _refusals(self, name, req):
        """The kernels against the windows, and what the device path leaves out: an external current, tensor-valued parameters."""
        yield self._kernel_refusal()
        if req.on_device:
            if name in req.inputs:
                yield NotImplementedError(f"bindsnet_amd: `inputs['{name}']`, an external current into a CSRMNodes layer, is not "
                                          "supported on the device")
            self._csrm_params({})                         # (raises what a tensor-valued parameter cannot run there)

    def _multi_device_refusal(self, mode, name):
        return NotImplementedError(f"{mode}: layer '{name}' (CSRMNodes) takes a window of currents and shares its threshold adaptation over the "
                                   "global batch, which the multi-device modes do not reproduce; run the network on one device")

    def _kernel_refusal(self):
        """What the reference's first step raises for this layer, found before a run changes any state: a response kernel that is
        not a vector (RectangularKernel: einsum on a 0-dim operand), kernels whose length is not the window's (dt != 1)."""
        try:
            wres, wref = self._window_sizes()
        except TypeError as e:
            return e
        if self.resKernel.dim() != 1 or self.refKernel.dim() != 1:
            return RuntimeError(f"einsum(): CSRMNodes.{self.responseKernel} gives a {self.resKernel.dim()}-dimensional response kernel, "
                                "the step contracts a vector over the window")
        if self.resKernel.numel() != wres or self.refKernel.numel() != wref:
            return RuntimeError(f"einsum(): the kernels of CSRMNodes have {self.resKernel.numel()} / {self.refKernel.numel()} entries at dt = "
                                f"{float(self.dt)}, the windows {wres} / {wref} slots (only dt = 1 runs)")
        if self.last_spikes.dim() < 2 or self.last_spikes.shape[1] != wref:
            return RuntimeError(f"CSRMNodes.last_spikes has shape {list(self.last_spikes.shape)}, the refractory window {wref} slots")
        return None

    def _csrm_params(self, pv: Optional[dict] = None) -> _lib.DcParams:
        self._scalars_only()
        p = _lib.DcParams()
        pv = {} if pv is None else pv
        p.lif = self._node_params(pv, decay=self.decay)
        p.theta_decay, p.theta_plus = self._sv("theta_decay", pv), self._sv("theta_plus", pv)
        p.learning, p.one_spike = int(self.learning), 0
        return p

    def _device_state(self, B: int):
        """The tensors snn_csrm_step reads beside `v`: (window-current buffer [B, Wres, n], last_spikes, resKernel, refKernel,
        Wres, Wref), each a contiguous f32 tensor on the layer's device.  Sizes beyond the kernels' limits raise.  The window-current
        buffer is scratch the layer keeps for itself (made anew for another batch size or device, never pickled), not state."""
        wres, wref = self._window_sizes()
        dev = self.v.device
        if max(wres, wref) > _lib.CSRM_MAX_WINDOW or B > 65535 or B * max(wres, wref) * self.n >= 1 << 31:
            raise NotImplementedError(f"bindsnet_amd: CSRMNodes with windows {wres} / {wref}, batch {B} and {self.n} neurons is beyond the device "
                                      f"kernels' limits (windows <= {_lib.CSRM_MAX_WINDOW}, batch <= 65535, batch * window * n < 2^31)")
        for name, shape in (("last_spikes", (B, wref, self.n)), ("resKernel", (wres,)), ("refKernel", (wref,))):
            t = getattr(self, name)
            if t.device != dev or t.dtype != torch.float32 or t.numel() != shape[0] * (shape[1] * shape[2] if len(shape) == 3 else 1) \
                    or not t.is_contiguous():
                raise ValueError(f"CSRMNodes.{name} must be a contiguous float32 tensor of {list(shape)} elements on {dev}")
        xwin = self.__dict__.get("_xwin")
        if xwin is None or xwin.device != dev or tuple(xwin.shape) != (B, wres, self.n):
            xwin = self.__dict__["_xwin"] = torch.zeros(B, wres, self.n, device=dev)
        return xwin, self.last_spikes, self.resKernel, self.refKernel, wres, wref

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_xwin", None)                          # device scratch, not model state
        return state

    def _describe(self, d, keep, scalars) -> int:
        pv = {}
        d.kind, d.p, d.theta = _lib.LAYER_CSRM, self._csrm_params(pv), _lib.dptr(self.theta)
        xwin, last, resk, refk, d.csrm_wres, d.csrm_wref = self._device_state(self.v.shape[0])
        d.csrm_xwin, d.csrm_last, d.csrm_resk, d.csrm_refk = _lib.dptr(xwin), _lib.dptr(last), _lib.dptr(resk), _lib.dptr(refk)
        keep.append(xwin)
        self._fill_pv(d, pv, keep)
        return 0

    def _host_step(self, x: torch.Tensor) -> None:
        from . import host_path
        host_path._step_csrm(self, x)

    def forward(self, x: torch.Tensor) -> None:
        """One step (nodes.py:1427-1464); `x` is the window of currents [B, res_window_size, *shape]."""
        if not self.v.is_cuda:
            return self._host_step(x)
        self._own_spikes()
        pv = {}
        p = self._csrm_params(pv)
        B = self.v.shape[0]
        _, last, resk, refk, wres, wref = self._device_state(B)
        x = x.to(torch.float32).contiguous()
        if x.numel() != B * wres * self.n:
            raise RuntimeError(f"CSRMNodes.forward: the input has shape {list(x.shape)}, the layer needs [{B}, {wres}, {self.n}]")
        ops.csrm_step(self.v, self.s, self.x if self.traces else None, self.theta, x, last, resk, refk, p, pv=pv)
