"""What Network.run knows about a call before it changes anything, handed to the `_refusals(key, request)` hook of every connection,
rule and layer.  Plain data plus lookups: what may not run is said by the classes, not here."""
from dataclasses import dataclass

import torch

from .monitors import Monitor, NetworkMonitor
from .nodes import Input


def is_analog(layer, x) -> bool:
    """Whether a run drives the Input `layer` with real values: a float32 entry of `inputs`, or a byte train behind a float32
    `s` that an analog run left and nobody reset -- connections read that `s` at t = 0, so the run is promoted to float32
    (exact: float32 zeros and ones give the bits their bytes give, include/snnhip.h f17)."""
    if x.dtype == torch.float32:
        return True
    left = getattr(layer, "s", None)
    return x.dtype in (torch.uint8, torch.bool) and isinstance(left, torch.Tensor) and left.dtype == torch.float32 \
        and left.numel() == x[0].numel() and bool(left.ne(0).any())


@dataclass(frozen=True)
class RunRequest:
    network: object
    inputs: dict                       # shapes normalised to [T, B, ...]
    T: int
    B: int                             # the batch size the run will have: the first input's
    on_device: bool
    learning: bool                     # network.learning and T > 0
    masks: dict
    injects_v: dict
    analog: dict                       # {name: input} of the Input layers a device run drives with real values

    @classmethod
    def of(cls, network, inputs, time, masks=None, injects_v=None, on_device=None) -> "RunRequest":
        T = int(time / network.dt)
        B = next((x.size(1) for x in inputs.values()), network.batch_size)
        on_device = network._device().type == "cuda" if on_device is None else on_device
        analog = {name: x for name, x in inputs.items() if on_device and isinstance(network.layers.get(name), Input) and is_analog(network.layers[name], x)}
        return cls(network, inputs, T, B, on_device, bool(network.learning and T > 0), masks or {}, injects_v or {}, analog)

    def feeders(self, name: str) -> list:
        """The connections filed as feeding the layer `name`."""
        return [conn for (_, dst), conn in self.network.connections.items() if dst == name]

    def readers(self, layer) -> list:
        """The connections whose source is `layer`."""
        return [conn for conn in self.network.connections.values() if getattr(conn, "source", None) is layer]

    def monitored(self, conn, key) -> bool:
        """Whether any monitor records a variable of this connection (its `activity` aside: that is a buffer of its own, not `w`)."""
        net = self.network
        return any((isinstance(m, Monitor) and m.obj is conn and not net._records_activity(m, conn)) or
                   (isinstance(m, NetworkMonitor) and any(c == key for c, _ in m._wanted_conns())) for m in net.monitors.values())

    def analog_source(self, conn):
        """(name, x) of the Input layer `conn` reads, where this run drives it with real values; else None."""
        return next(((name, x) for name, x in self.analog.items() if self.network.layers[name] is getattr(conn, "source", None)), None)
