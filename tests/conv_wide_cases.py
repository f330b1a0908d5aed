"""The wide-convolution fixture cases (tests/golden/make_golden_conv_wide.py), written once for both implementations: `build(ns, name)`
constructs a case's network from a namespace of classes -- the reference's (the generator) or this package's (the tests) -- and
`run_case` drives it and records, per input, every non-Input layer's raster and state in full.

A Conv2dConnection with more than 16 input channels is summed by the device in the stated order (include/snnhip.h,
snn_prop_conv2d_f32) and by the reference in whatever blocked order its oneDNN picks on the host.  Every weight and bias here is a
multiple of 1/64 in [-1, 1] and no output sums more than 2048 taps: every partial sum, in ANY order, is a multiple of 2^-6 below
2^12, i.e. fits 18 of f32's 24 bits -- no addition rounds, so both orders give the same bits and the fixtures carry bit-exact parity
with the unmodified reference (`assert_grid`, called on every network built).

(a) Input [32, 6, 7] -> Conv2d(32 -> 9, k3, s1, p1) -> LIFNodes; B 3, T 30, 20 % input density
(b) Input [17, 5, 5] -> Conv2d(17 -> 4, k3, s2, p0) -> IFNodes; B 1
(c) Input [3, 8, 8] -> Conv2d(3 -> 20, k3, p1) -> SubtractiveResetIFNodes -> MaxPool2dConnection(2, 2) -> PassThroughNodes
    -> Conv2d(20 -> 24, k3, p1) -> SubtractiveResetIFNodes; B 2
(d) ann_to_snn of Sequential(Conv2d(1, 20, 3), ReLU, Conv2d(20, 24, 3), ReLU, Linear(384, 5)) on a (1, 8, 8) input, every `w` and `b`
    snapped to the grid after the conversion (`snap`); B 2
(e) (a) at dt = 0.5"""
import hashlib
import warnings
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from conversion_cases import set_batch, snapshot
from dt_cases import run_time

f32 = np.float32
GRID = 64
MAX_TAPS = 2048
T, N_IN = 30, 2
RATE_BAND = (0.02, 0.40)          # every spiking layer's share of neuron-steps with a spike, in the reference (asserted by the generator)

CASES = {
    "a": dict(kind="single", shape=(32, 6, 7), cout=9, k=3, s=1, p=1, nodes="LIF", B=3, density=0.2, dt=1.0, w=(-24, 40), thresh=-52.0),
    "b": dict(kind="single", shape=(17, 5, 5), cout=4, k=3, s=2, p=0, nodes="IF", B=1, density=0.2, dt=1.0, w=(-24, 40), thresh=-52.0),
    "c": dict(kind="two", shape=(3, 8, 8), mid=20, cout=24, B=2, density=0.2, dt=1.0, w1=(-16, 48), w2=(-32, 32), thresh1=6.0, thresh2=8.0),
    "d": dict(kind="ann", shape=(1, 8, 8), B=2, density=0.3, dt=1.0),
}
CASES["e"] = dict(CASES["a"], dt=0.5, sibling="a")
NAMES = list(CASES)
ANN_BANDS = [(-16, 32), (-8, 8), (-8, 8), (0, 16), (-4, 4), (0, 16)]             # (d): weight and bias of each layer, in 1/64


def ns_from(nodes, topology, network_cls, monitor_cls, conversion):
    return SimpleNamespace(Input=nodes.Input, IFNodes=nodes.IFNodes, LIFNodes=nodes.LIFNodes, Connection=topology.Connection,
                           Conv2dConnection=topology.Conv2dConnection, MaxPool2dConnection=topology.MaxPool2dConnection,
                           Network=network_cls, Monitor=monitor_cls, SIF=conversion.SubtractiveResetIFNodes, Pass=conversion.PassThroughNodes,
                           ann_to_snn=conversion.ann_to_snn)


def seed_of(name):
    return 900 + NAMES.index(CASES[name].get("sibling", name))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def grid(rng, lo, hi, *shape):
    """Multiples of 1/64 between lo/64 and hi/64."""
    return torch.from_numpy((rng.integers(lo, hi + 1, size=shape) / float(GRID)).astype(f32))


def snap(net):
    """Every Conv2dConnection's and Connection's `w` and `b` to the nearest multiple of 1/64 inside [-1, 1], in place."""
    with torch.no_grad():
        for conn in net.connections.values():
            for p in (getattr(conn, "w", None), getattr(conn, "b", None)):
                if p is not None:
                    p.copy_((torch.round(p * GRID) / GRID).clamp_(-1.0, 1.0))
    return net


def assert_grid(net):
    """What makes every partial sum exact: grid weights within [-1, 1], at most MAX_TAPS terms per output (2048 * 64 + 64 < 2^24)."""
    seen = 0
    for conn in net.connections.values():
        w = getattr(conn, "w", None)
        if w is None:
            continue
        seen += 1
        for p in (w, getattr(conn, "b", None)):
            if p is not None:
                a = p.detach().cpu().numpy().astype(np.float64) * GRID
                assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= GRID, "a weight or bias off the 1/64 grid or outside [-1, 1]"
        terms = int(np.prod(w.shape[1:])) if w.dim() == 4 else int(w.shape[0])
        assert terms <= MAX_TAPS, terms
    assert seen > 0
    return net


def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def make_ann(name):
    rng = np.random.default_rng(seed_of(name))
    ann = nn.Sequential(nn.Conv2d(1, 20, 3), nn.ReLU(), nn.Conv2d(20, 24, 3), nn.ReLU(), nn.Linear(24 * 4 * 4, 5))
    with torch.no_grad():
        for p, (lo, hi) in zip(ann.parameters(), ANN_BANDS):
            p.copy_(grid(rng, lo, hi, *p.shape) + 0.003)                           # (off the grid: `snap` has something to do)
    return ann


def build(ns, name, eval_mode=False):
    """The case's network.  eval_mode: network.train(False) -- the generator's call: in training mode the reference's NoOp multiplies
    the `w` a pooling connection does not have; this package runs them in training mode, so the tests do not."""
    c = CASES[name]
    rng = np.random.default_rng(seed_of(name))
    torch.manual_seed(seed_of(name))
    if c["kind"] == "ann":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            net = ns.ann_to_snn(make_ann(name), c["shape"])
        set_batch(net, c["B"])
        snap(net)
    else:
        net = ns.Network(dt=c["dt"], batch_size=c["B"])
        cin, h, w = c["shape"]
        net.add_layer(ns.Input(shape=c["shape"]), name="X")
        if c["kind"] == "single":
            oh, ow = conv_out(h, c["k"], c["s"], c["p"]), conv_out(w, c["k"], c["s"], c["p"])
            cls = {"LIF": ns.LIFNodes, "IF": ns.IFNodes}[c["nodes"]]
            net.add_layer(cls(shape=(c["cout"], oh, ow), traces=True, thresh=c["thresh"], refrac=2), name="Y")
            net.add_connection(ns.Conv2dConnection(net.layers["X"], net.layers["Y"], kernel_size=c["k"], stride=c["s"], padding=c["p"],
                                                   w=grid(rng, *c["w"], c["cout"], cin, c["k"], c["k"]), b=grid(rng, -32, 32, c["cout"])), "X", "Y")
        else:
            net.add_layer(ns.SIF(shape=(c["mid"], h, w), thresh=c["thresh1"], reset=0.0, refrac=0), name="C1")
            net.add_layer(ns.Pass(shape=(c["mid"], h // 2, w // 2)), name="P")
            net.add_layer(ns.SIF(shape=(c["cout"], h // 2, w // 2), thresh=c["thresh2"], reset=0.0, refrac=0), name="Y")
            net.add_connection(ns.Conv2dConnection(net.layers["X"], net.layers["C1"], kernel_size=3, padding=1,
                                                   w=grid(rng, *c["w1"], c["mid"], cin, 3, 3), b=grid(rng, -16, 16, c["mid"])), "X", "C1")
            net.add_connection(ns.MaxPool2dConnection(net.layers["C1"], net.layers["P"], kernel_size=2, stride=2, decay=1), "C1", "P")
            net.add_connection(ns.Conv2dConnection(net.layers["P"], net.layers["Y"], kernel_size=3, padding=1,
                                                   w=grid(rng, *c["w2"], c["cout"], c["mid"], 3, 3), b=grid(rng, -16, 16, c["cout"])), "P", "Y")
    if eval_mode:
        net.train(False)
    return assert_grid(net)


def input_name(net):
    return next(iter(net.layers))          # "X", or ann_to_snn's "Input"


def inputs(name, r):
    """Input `r` of a case: [T, B, *shape] uint8 from numpy's generator."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * seed_of(name) + r)
    return (rng.random((T, c["B"], *c["shape"])) < c["density"]).astype(np.uint8)


def wide(net):
    """The network's Conv2dConnections with more than 16 input channels."""
    return [c for c in net.connections.values() if type(c).__name__ == "Conv2dConnection" and c.source.shape[0] > 16]


def weights_sha(net):
    return [sha(p.detach().cpu().numpy()) for conn in net.connections.values() for p in (getattr(conn, "w", None), getattr(conn, "b", None))
            if p is not None]


def run_case(ns, net, name, device=None, first=0, count=None, halves=False):
    """Run inputs [first, first + count) with reset_state_variables() between them; one snapshot per input (conversion_cases.snapshot:
    `<layer>_raster`, `_v`, `_rc`, `_x`, `_summed`, `<layer>_fr` of a pooling connection).  halves: every input as two runs under one monitor."""
    c = CASES[name]
    B, dt, inp = c["B"], c["dt"], input_name(net)
    count = N_IN - first if count is None else count
    out = []
    for r in range(first, first + count):
        mons = {l: ns.Monitor(layer, ["s"], time=T) for l, layer in net.layers.items() if l != inp}
        for l, m in mons.items():
            net.add_monitor(m, name=l + "_s")
        x = torch.from_numpy(inputs(name, r))
        if device is not None:
            x = x.to(device)
        if halves:
            h = T // 2
            net.run({inp: x[:h].clone()}, time=run_time(h, dt))
            net.run({inp: x[h:].clone()}, time=run_time(T - h, dt))
        else:
            net.run({inp: x}, time=run_time(T, dt))
        rasters = {l: (m.get("s").cpu().numpy().reshape(T, B, -1) != 0).astype(np.uint8) for l, m in mons.items()}
        out.append(snapshot(net, rasters, {}))
        for l in mons:
            del net.monitors[l + "_s"]
        net.reset_state_variables()
    return out


def spiking_layers(net):
    return [l for l, layer in net.layers.items() if hasattr(layer, "refrac_count")]
