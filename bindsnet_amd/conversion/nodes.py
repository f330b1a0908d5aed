"""The two layer classes of bindsnet.conversion (reference: bindsnet/conversion/nodes.py): `SubtractiveResetIFNodes`, the
integrate-and-fire neuron a converted ANN is made of, and `PassThroughNodes`, which hands its input on as its spikes.  On the
device their steps are snn_sif_step / snn_pass_step of libsnnhip (csrc/snn_conversion.hip), driven by Network.run's generic plan;
on the host the reference's own torch calls (network/host_path.py)."""
from typing import Iterable, Optional, Union

import torch

from .. import _lib, ops
from ..network.nodes import Nodes, Scalar, _buf, _f


class SubtractiveResetIFNodes(Nodes):
    """Integrate-and-fire neurons that are reset by subtraction (reference: conversion/nodes.py:8-119): a neuron that crosses its
    threshold keeps what it holds above it, `v -= thresh`; `reset` is only where reset_state_variables() and set_batch_size() put
    the voltage.  The refractory gate is `refrac_count == 0`, and the counter is `(refrac_count > 0) * (refrac_count - dt)`.

    The only class that takes `sum_input=True`: `summed` [B, *shape] then adds up the layer's raw input of every step -- the
    readout of a network made by `ann_to_snn`.  On the device `thresh`, `reset`, `refrac` and `lbound` must be scalars (the
    reference's `v[s] - thresh` cannot broadcast a tensor either); `tc_trace` / `trace_scale` may be per-neuron tensors as on
    every class."""
    _SUMS_INPUT = True
    _SCALAR_ONLY = ("thresh", "reset", "refrac", "lbound")      # refused as tensors on the device, by name
    _WATCHED = ("summed",)

    def _multi_device_refusal(self, mode, name):
        """bindsnet.conversion's layers run on the generic plan of one device only."""
        return NotImplementedError(f"{mode}: layer '{name}' ({type(self).__name__}) is not supported by the multi-device modes; "
                                   "run the network on one device")

    def __init__(self, n: Optional[int] = None, shape: Optional[Iterable[int]] = None, traces: bool = False,
                 traces_additive: bool = False, tc_trace: Scalar = 20.0, trace_scale: Scalar = 1.0, sum_input: bool = False,
                 thresh: Scalar = -52.0, reset: Scalar = -65.0, refrac: Union[int, torch.Tensor] = 5, lbound: float = None,
                 **kwargs) -> None:
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
        self._scalars_only()
        return self._node_params(pv, reset=self.reset, refrac=self.refrac)

    def _summed(self) -> Optional[torch.Tensor]:
        """`summed` as the step kernel adds to it: a contiguous f32 [B, *shape] tensor beside `v`, or None without sum_input."""
        if not self.sum_input:
            return None
        t = self.summed
        if t.device != self.v.device or t.dtype != torch.float32 or t.shape != self.v.shape or not t.is_contiguous():
            raise ValueError(f"layer state 'summed' must be a contiguous float32 {list(self.v.shape)} tensor on {self.v.device}")
        return t

    def _describe(self, d, keep, scalars) -> int:
        pv = {}
        d.kind, d.p.lif = _lib.LAYER_SIF, self._params(pv)
        d.summed = _lib.dptr(self._summed())
        self._fill_pv(d, pv, keep)
        return 0

    def _host_step(self, x: torch.Tensor) -> None:
        from ..network import host_path
        host_path._step_sif(self, x)

    def forward(self, x: torch.Tensor) -> None:
        """One step (conversion/nodes.py:73-99)."""
        if not self.v.is_cuda:
            return self._host_step(x)
        self._own_spikes()
        pv = {}
        p = self._params(pv)
        ops.sif_step(self.v, self.refrac_count, self.s, self.x if self.traces else None, x.to(torch.float32).contiguous(), p,
                     summed=self._summed(), pv=pv)


class PassThroughNodes(Nodes):
    """A layer whose spikes are its input (reference: conversion/nodes.py:122-176): the target of the pooling, permuting and
    padding connections of a converted network.  `forward(x)` is `s = x` and nothing else -- no trace and no `summed`, whatever
    the constructor was told, because the reference never reaches the base class's step; reset_state_variables() zeroes `s`
    only; `v` is zeros(shape) without a batch dimension and never changes.

    On the host `s` is the float32 input tensor itself.  On the device the layer keeps `s` as a bool [B, *shape] tensor with the
    same values (a deviation in dtype only), and is accepted only where exactly one connection feeds it and that connection is
    a MaxPool1d/2d/3dConnection, PermuteConnection or ConstantPad2dConnection, whose outputs are 0 or 1: anything else -- another
    connection class, a second incoming connection, an external current, `injects_v` -- raises NotImplementedError before the
    run changes state (`_refusals`)."""
    _STATE = ()
    _WATCHED = ("v",)
    _multi_device_refusal = SubtractiveResetIFNodes._multi_device_refusal

    def _recordable(self) -> tuple:
        return ()                                         # (no step writes `x`: see _describe)

    def __init__(self, n: Optional[int] = None, shape: Optional[Iterable[int]] = None, traces: bool = False,
                 traces_additive: bool = False, tc_trace: Scalar = 20.0, trace_scale: Scalar = 1.0, sum_input: bool = False) -> None:
        super().__init__(n=n, shape=shape, traces=traces, traces_additive=traces_additive, tc_trace=tc_trace,
                         trace_scale=trace_scale, sum_input=sum_input)
        self.register_buffer("v", torch.zeros(*self.shape))

    def reset_state_variables(self) -> None:
        self.s.zero_()

    def _refusals(self, name, req):
        if req.on_device:
            yield self._run_refusal(name, req.feeders(name), name in req.inputs, req.injects_v.get(name) is not None)

    def _run_refusal(self, name: str, feeders: list, has_current: bool, injected: bool):
        """Why a device run must not start with this layer in it, or None.  `feeders`: the connections into the layer."""
        from ..network.topology import _MaxPoolConnection
        from .topology import ConstantPad2dConnection, PermuteConnection
        if has_current:
            return NotImplementedError(f"bindsnet_amd: `inputs['{name}']`, an external current into a PassThroughNodes layer, is not "
                                       "supported on the device (its spikes are kept as 0 / 1 bytes)")
        if injected:
            return NotImplementedError(f"bindsnet_amd: injects_v['{name}'] on a PassThroughNodes layer is not supported on the device (its "
                                       "`v` has no batch dimension and never changes)")
        if len(feeders) != 1:
            return NotImplementedError(f"bindsnet_amd: PassThroughNodes layer '{name}' needs exactly one incoming connection on the "
                                       f"device, it has {len(feeders)}")
        if not isinstance(feeders[0], (_MaxPoolConnection, PermuteConnection, ConstantPad2dConnection)):
            return NotImplementedError(f"bindsnet_amd: {type(feeders[0]).__name__} into PassThroughNodes layer '{name}' is not supported on "
                                       "the device: its spikes are kept as 0 / 1 bytes, which only MaxPool1d/2d/3dConnection, PermuteConnection "
                                       "and ConstantPad2dConnection are known to feed")
        return None

    def _describe(self, d, keep, scalars) -> int:
        d.kind = _lib.LAYER_PASS
        d.p.lif.traces = 0                                # (traces=True makes the buffers, but no step ever writes them)
        d.v = d.x = None
        return 0

    def _host_step(self, x: torch.Tensor) -> None:
        self.s = x

    def forward(self, x: torch.Tensor) -> None:
        """One step (conversion/nodes.py:161-169)."""
        if not x.is_cuda:
            return self._host_step(x)
        if self.s.dtype != torch.bool or self.s.shape != x.shape or self.s.device != x.device:
            self.s = torch.zeros(x.shape, dtype=torch.bool, device=x.device)
        ops.pass_step(self.s, x.to(torch.float32).contiguous())
