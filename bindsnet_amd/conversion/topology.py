"""The two connection classes of bindsnet.conversion (reference: bindsnet/conversion/topology.py): `PermuteConnection` and
`ConstantPad2dConnection`, which re-arrange the source's spikes on their way to a PassThroughNodes layer.  Neither has weights.
On the device both are one gather whose source index is computed from at most three extents and strides
(snn_prop_gather_f32, csrc/snn_conversion.hip); on the host the reference's own torch calls (network/host_path.py)."""
from typing import Iterable, Tuple

import torch

from .. import _lib, ops
from ..network import host_path
from ..network.nodes import Nodes
from ..network.topology import _FixedConnection


class _GatherConnection(_FixedConnection):
    """What the two classes share.  No `w`: nothing learns (a rule other than NoOp raises in the rule's constructor), nothing is
    normalised, a mask or a monitor on the connection raises before the run, as for the MaxPoolNdConnection classes; like those
    the connection runs in training mode, and parallel.py's multi-device modes refuse it by name."""

    def _geometry(self):
        """(arrays of snn_prop_gather_f32, the shape of one output sample); raises what the class cannot run on the device."""
        raise NotImplementedError

    def _checked_geometry(self):
        arrays, out = self._geometry()
        if tuple(out) != tuple(self.target.shape):
            raise RuntimeError(f"{type(self).__name__}: the connection's output has shape {tuple(out)} per sample, the target "
                               f"{tuple(self.target.shape)}")
        return arrays, out

    def _run_refusal(self, mask, monitored: bool):
        if mask is not None:
            return NotImplementedError(f"bindsnet_amd: a mask on a {type(self).__name__} is not supported (it has no weights)")
        if monitored:
            return NotImplementedError(f"bindsnet_amd: a monitor on a {type(self).__name__} is not supported (it has no state)")
        return None

    def _refusals(self, key, req):
        yield from super()._refusals(key, req)
        if req.on_device:
            self._checked_geometry()                      # (raises what the device cannot gather; the host path runs torch's own calls)

    def compute(self, s: torch.Tensor) -> torch.Tensor:
        if not s.is_cuda:
            return self._host_compute(s)
        arrays, out_shape = self._geometry()
        out = torch.empty(s.size(0), *out_shape, device=s.device)
        ops.prop_gather(self._spike_bytes(s), out, arrays)
        return out

    @staticmethod
    def _spike_bytes(s: torch.Tensor) -> torch.Tensor:
        if s.dtype not in (torch.bool, torch.uint8):
            raise NotImplementedError(f"bindsnet_amd: float-valued (analog) spikes are not supported on the device (got {s.dtype})")
        return s.contiguous()

    def _prop_into(self, s, out, accumulate=False) -> None:
        arrays, _ = self._checked_geometry()
        ops.prop_gather(self._spike_bytes(s), out, arrays, accumulate=accumulate)

    def _describe(self, d, B, dev, scratch):
        arrays, _ = self._checked_geometry()
        d.kind, d.w = self._kind, None
        for name, arr in zip(("gat_out", "gat_src", "gat_stride", "gat_off"), arrays):
            for a in range(3):
                getattr(d, name)[a] = arr[a]
        return []


class PermuteConnection(_GatherConnection):
    """`compute(s)` is `s.permute(dims).float()` over [B, *source.shape] (reference: conversion/topology.py:9-56), so `dims`
    names the batch dimension too.  On the device the batch stays in front (`dims[0] == 0`), the source has at most three
    dimensions, and the permuted shape must be the target's: NotImplementedError / RuntimeError before the run otherwise."""

    _kind = _lib.CONN_PERMUTE
    _host_compute = host_path._propagate_permute

    def __init__(self, source: Nodes, target: Nodes, dims: Iterable, nu=None, weight_decay: float = 0.0, **kwargs) -> None:
        super().__init__(source, target, nu, None, weight_decay, **kwargs)
        self.dims = dims

    def _geometry(self):
        dims, rank = [int(d) for d in self.dims], len(self.source.shape)
        if rank > 3:
            raise NotImplementedError(f"bindsnet_amd: PermuteConnection over a source of {rank} dimensions is not supported on the "
                                      "device (at most three)")
        if sorted(dims) != list(range(rank + 1)):
            raise RuntimeError(f"PermuteConnection: dims {tuple(dims)} is not a permutation of the {rank + 1} dimensions of "
                               "[batch, *source.shape] (torch's permute raises the same)")
        if dims[0] != 0:
            raise NotImplementedError(f"bindsnet_amd: PermuteConnection with dims {tuple(dims)} moves the batch dimension, which is not "
                                      "supported on the device (dims[0] must be 0)")
        return ops.permute_geometry(self.source.shape, [d - 1 for d in dims[1:]])


class ConstantPad2dConnection(_GatherConnection):
    """`compute(s)` is `F.pad(s, padding).float()` (reference: conversion/topology.py:59-108).  The fill is always 0: the reference
    does not look at ConstantPad2d.value, and neither does this class.  On the device `padding` is four non-negative ints (left,
    right, top, bottom of the last two dimensions) and the padded shape must be the target's; negative padding -- cropping --
    raises NotImplementedError."""

    _kind = _lib.CONN_PAD
    _host_compute = host_path._propagate_pad

    def __init__(self, source: Nodes, target: Nodes, padding: Tuple, nu=None, weight_decay: float = 0.0, **kwargs) -> None:
        super().__init__(source, target, nu, None, weight_decay, **kwargs)
        self.padding = padding

    def _geometry(self):
        pad, rank = self.padding, len(self.source.shape)
        if not isinstance(pad, (tuple, list)) or len(pad) != 4 or any(isinstance(p, bool) or not isinstance(p, int) for p in pad):
            raise NotImplementedError(f"bindsnet_amd: ConstantPad2dConnection needs `padding` as a 4-tuple of ints on the device, got {pad!r}")
        if min(pad) < 0:
            raise NotImplementedError(f"bindsnet_amd: ConstantPad2dConnection with negative padding {tuple(pad)} (cropping) is not supported "
                                      "on the device")
        if rank < 2 or rank > 3:
            raise NotImplementedError(f"bindsnet_amd: ConstantPad2dConnection over a source of {rank} dimensions is not supported on the "
                                      "device (two or three: the last two are padded)")
        lead = (0,) * (rank - 2)
        return ops.pad_geometry(self.source.shape, lead + (pad[2], pad[0]), lead + (pad[3], pad[1]))
