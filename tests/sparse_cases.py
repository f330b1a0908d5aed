"""The SparseConnection fixture cases (tests/golden/make_golden_sparse.py), written once for both implementations: `build(ns, case)`
constructs a case's network from a namespace of classes -- the reference's (the generator) or this package's (the tests) -- and
`run_case` drives it and records, after every input, the Y raster, v, refrac_count, theta (where the layer has one), both traces
and the global generator's position.  Every connection is a SparseConnection: its sums are the reference's own bit for bit, float
weights included, which a dense Connection's are not.

(a) Input 100 -> Sparse (20 % dense, w = 3 * rand) -> LIF 50; batch 1, 50 steps, 2 inputs
(b) Input 64 -> Sparse (no `w` given: the constructor's own draw between wmin 0 and wmax 0.6, every entry stored) -> LIF 300, plus a
    recurrent Sparse 300 -> 300 (5 %, signed weights, bias `b`); batch 3, 40 steps
(c) Input 1100 -> Sparse (0.5 %) -> LIF 37; batch 33, 30 steps.  Most rows are empty; row 1030 (behind the 1024-source chunk
    boundary) holds every column that has entries at all; columns 5 and 20 are empty; column 36, the last of an odd count, holds one
    entry only
(d) Inputs X1 (40) and X2 (90), each -> Sparse -> the same LIF 70, plus a recurrent Sparse; connections added in the order X2 -> Y,
    Y -> Y, X1 -> Y (the sums of one target accumulate in that order); X1 -> Y is given a `w` that wmax = 1 clamps; batch 2
(e) an all-zero `w` (no stored entry) with a bias; batch 2
(f) (a) with a DiehlAndCookNodes target (one_spike draws from the global generator) and network.train(True): the reference's
    NoOp multiplies `w` by 1.0 every step
(g) Input 2500 -> Sparse (2 %) -> LIF 700; batch 2, 20 steps: three column tiles, three source chunks"""
import hashlib
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time

CASES = {
    "a": dict(inputs={"X": 100}, n=50, node="lif", B=1, T=50, n_in=2, rate=0.1, seed=21,
              conns=[dict(src="X", dst="Y", density=0.2, scale=3.0)]),
    "b": dict(inputs={"X": 64}, n=300, node="lif", B=3, T=40, n_in=2, rate=0.15, seed=22,
              conns=[dict(src="X", dst="Y", drawn=True, wmin=0.0, wmax=0.6),
                     dict(src="Y", dst="Y", density=0.05, scale=4.0, signed=True, bias=0.5)]),
    "c": dict(inputs={"X": 1100}, n=37, node="lif", B=33, T=30, n_in=2, rate=0.05, seed=23,
              conns=[dict(src="X", dst="Y", density=0.005, scale=30.0, carve=True)]),
    "d": dict(inputs={"X1": 40, "X2": 90}, n=70, node="lif", B=2, T=40, n_in=2, rate=0.1, seed=24,
              conns=[dict(src="X2", dst="Y", density=0.1, scale=3.0),
                     dict(src="Y", dst="Y", density=0.1, scale=3.0, signed=True),
                     dict(src="X1", dst="Y", density=0.3, scale=2.0, wmax=1.0)]),
    "e": dict(inputs={"X": 30}, n=20, node="lif", B=2, T=40, n_in=2, rate=0.2, seed=25,
              conns=[dict(src="X", dst="Y", density=0.0, scale=1.0, bias=1.0)]),
    "f": dict(inputs={"X": 100}, n=50, node="dc", B=1, T=50, n_in=2, rate=0.1, seed=21, train=True,
              conns=[dict(src="X", dst="Y", density=0.2, scale=3.0)]),
    "g": dict(inputs={"X": 2500}, n=700, node="lif", B=2, T=20, n_in=2, rate=0.05, seed=27,
              conns=[dict(src="X", dst="Y", density=0.02, scale=3.0)]),
}
# (d) at dt = 0.5 (default 1.0; `time = T * dt` is run): the refractory countdown and the decays of the generic plan's LIF step behind
# the sparse propagation.  `sibling`: the dt = 1 case it repeats.
CASES["d_dt05"] = dict(CASES["d"], dt=0.5, sibling="d")


def ns_from(nodes, topology, network_cls):
    return SimpleNamespace(Input=nodes.Input, LIFNodes=nodes.LIFNodes, DiehlAndCookNodes=nodes.DiehlAndCookNodes,
                           SparseConnection=topology.SparseConnection, Network=network_cls)


def dense_weights(name, k, n_src, n_dst):
    """The dense [n_src, n_dst] matrix connection k of the case is given (None: the constructor draws it), and its bias or None.
    Exact zeros are what `to_sparse()` drops."""
    c = CASES[name]
    spec = c["conns"][k]
    g = torch.Generator().manual_seed(1000 * c["seed"] + k)
    bias = None
    if spec.get("bias") is not None:
        bias = spec["bias"] * torch.rand(n_dst, generator=g)
    if spec.get("drawn"):
        return None, bias
    w = spec["scale"] * torch.rand(n_src, n_dst, generator=g)
    if spec.get("signed"):
        w = w - 0.5 * spec["scale"]
    w = w * (torch.rand(n_src, n_dst, generator=g) < spec["density"])
    if spec.get("carve"):                        # case (c)'s rows and columns
        w[1030] = spec["scale"] * (0.25 + torch.rand(n_dst, generator=g))
        w[:1030, 36] = 0.0
        w[1031:, 36] = 0.0
        w[:, 5] = 0.0
        w[:, 20] = 0.0
    return w.contiguous(), bias


def build(ns, name):
    """The case's network (a connection without a given `w` draws it from the global generator after torch.manual_seed(seed))."""
    c = CASES[name]
    torch.manual_seed(c["seed"])
    net = ns.Network(dt=c.get("dt", 1.0))
    sizes = dict(c["inputs"], Y=c["n"])
    for lname, n in c["inputs"].items():
        net.add_layer(ns.Input(n=n, traces=True), name=lname)
    net.add_layer((ns.LIFNodes if c["node"] == "lif" else ns.DiehlAndCookNodes)(n=c["n"], traces=True), name="Y")
    for k, spec in enumerate(c["conns"]):
        w, b = dense_weights(name, k, sizes[spec["src"]], sizes[spec["dst"]])
        kw = {key: spec[key] for key in ("wmin", "wmax") if key in spec}
        if w is not None:
            kw["w"] = w
        if b is not None:
            kw["b"] = b
        conn = ns.SparseConnection(net.layers[spec["src"]], net.layers[spec["dst"]], **kw)
        net.add_connection(conn, source=spec["src"], target=spec["dst"])
    if c.get("train"):
        net.train(True)
    return net


def inputs(name, r):
    """Input `r` of a case: {layer: [T, B, n] uint8} from numpy's generator."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c["seed"] + r + 7)
    return {lname: (rng.random((c["T"], c["B"], n)) < c["rate"]).astype(np.uint8) for lname, n in c["inputs"].items()}


def generator_probe():
    """Four draws of the global generator, which is left where it was: pins its position after a run."""
    state = torch.get_rng_state()
    v = torch.rand(4).numpy().copy()
    torch.set_rng_state(state)
    return v


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def weights_sha(net):
    """sha256 of every connection's dense weights, in connection order."""
    return [sha(conn.w.detach().to_dense().cpu().numpy().astype(np.float32)) for conn in net.connections.values()]


def snapshot(net, raster):
    Y = net.layers["Y"]
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).copy()       # noqa: E731
    out = dict(raster=np.asarray(raster, np.uint8), v=f(Y.v), refrac=f(Y.refrac_count), xY=f(Y.x), gen=generator_probe())
    if hasattr(Y, "theta"):
        out["theta"] = f(Y.theta)
    for lname in net.layers:
        if lname != "Y":
            out["x" + lname] = f(net.layers[lname].x)
    return out


def run_case(net, name, monitor_cls, device=None, first=0, count=None):
    """Run inputs [first, first+count) of the case (reset_state_variables() between them); returns one snapshot per input."""
    c = CASES[name]
    out = []
    count = c["n_in"] - first if count is None else count
    for r in range(first, first + count):
        mon = monitor_cls(net.layers["Y"], ["s"], time=c["T"])
        net.add_monitor(mon, name="Y_s")
        x = {k: torch.from_numpy(v) for k, v in inputs(name, r).items()}
        if device is not None:
            x = {k: v.to(device) for k, v in x.items()}
        net.run(x, time=run_time(c["T"], c.get("dt", 1.0)))
        raster = mon.get("s").cpu().numpy().reshape(c["T"], c["B"], -1).astype(np.uint8)
        out.append(snapshot(net, raster))
        del net.monitors["Y_s"]
        net.reset_state_variables()
    return out
