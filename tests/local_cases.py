"""The locally connected fixture cases (tests/golden/make_golden_local.py), written once for both implementations: `build(ns,
case)` constructs a case's network from a namespace of classes -- the reference's (the generator) or this package's (the
tests) -- and `run_case` drives it and records, after every input, the Y raster, v, refrac_count, theta, both traces and w.

(a) the loc2d_mnist.py graph: Input [1, 20, 20] -> LocalConnection2D (k 12, s 4, 50 filters, PostPre nu = (1e-4, 1e-2),
    wmin 0, wmax 1, norm 0.2*144) -> AdaptiveLIFNodes [50, 3, 3] (reset -60, tc_theta_decay 1e6) with the -25 recurrent
    inhibition between receptive-field partners; 3 inputs x 100 steps, 5 % input density, batch 1
(b) LocalConnection2D, 2 input channels, 9 x 11 input, kernel (4, 3), stride (2, 3), batch 3
(c) LocalConnection1D, 2 input channels, batch 2
(d) LocalConnection3D at batch 1
(e) (a) with network.train(False)
(f) AdaptiveLIFNodes behind a plain Connection (weights on a 1/4 grid, so every current is exact in any order)"""
import hashlib
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time

CASES = {
    "a": dict(kind="lc2d", cin=1, shape=(20, 20), k=12, s=4, F=50, B=1, T=100, n_in=3, density=0.05, nu=(1e-4, 1e-2),
              norm=0.2 * 144, inh=25.0, train=True, seed=0),
    "b": dict(kind="lc2d", cin=2, shape=(9, 11), k=(4, 3), s=(2, 3), F=3, B=3, T=40, n_in=2, density=0.3, nu=(1e-2, 2e-2),
              norm=None, inh=0.0, train=True, seed=1),
    "c": dict(kind="lc1d", cin=2, shape=(30,), k=5, s=3, F=4, B=2, T=40, n_in=2, density=0.3, nu=(1e-2, 2e-2),
              norm=None, inh=0.0, train=True, seed=2),
    "d": dict(kind="lc3d", cin=1, shape=(6, 6, 6), k=3, s=2, F=3, B=1, T=40, n_in=2, density=0.3, nu=(1e-2, 2e-2),
              norm=0.5 * 27, inh=0.0, train=True, seed=3),
    "e": dict(kind="lc2d", cin=1, shape=(20, 20), k=12, s=4, F=50, B=1, T=100, n_in=3, density=0.05, nu=(1e-4, 1e-2),
              norm=0.2 * 144, inh=25.0, train=False, seed=0),
    "f": dict(kind="dense", cin=1, shape=(50,), F=30, B=2, T=60, n_in=2, density=0.2, train=True, seed=4),
}
# (b) at dt = 0.5 (default 1.0; `time = T * dt` is run): the refractory countdown, the decays of v / theta / both traces.  `sibling`:
# the dt = 1 case it repeats.
CASES["b_dt05"] = dict(CASES["b"], dt=0.5, sibling="b")


def ns_from(nodes, topology, learning, network_cls):
    return SimpleNamespace(Input=nodes.Input, AdaptiveLIFNodes=nodes.AdaptiveLIFNodes, Connection=topology.Connection,
                           LocalConnection1D=topology.LocalConnection1D, LocalConnection2D=topology.LocalConnection2D,
                           LocalConnection3D=topology.LocalConnection3D, PostPre=learning.PostPre, Network=network_cls)


def _conv(n, k, s):
    return int((n - k) / s) + 1


def target_shape(c):
    if c["kind"] == "dense":
        return [c["F"]]
    ks = c["k"] if isinstance(c["k"], tuple) else (c["k"],) * len(c["shape"])
    ss = c["s"] if isinstance(c["s"], tuple) else (c["s"],) * len(c["shape"])
    conv = [_conv(n, k, s) for n, k, s in zip(c["shape"], ks, ss)]
    return [c["F"], int(np.prod(conv))] if c["kind"] == "lc1d" else [c["F"]] + conv


def build(ns, name):
    """The case's network (weights drawn from the global generator after torch.manual_seed(seed))."""
    c = CASES[name]
    torch.manual_seed(c["seed"])
    net = ns.Network(dt=c.get("dt", 1.0))
    X = ns.Input(shape=[c["cin"], *c["shape"]], traces=True, tc_trace=20.0)
    if c["kind"] == "dense":
        Y = ns.AdaptiveLIFNodes(n=c["F"], traces=True, rest=-65.0, reset=-60.0, thresh=-58.0, refrac=3, tc_trace=20.0,
                                theta_plus=0.5, tc_theta_decay=200.0, lbound=-70.0)
        w = torch.from_numpy(np.random.default_rng(c["seed"]).integers(0, 8, (X.n, Y.n)).astype(np.float32) * 0.25)
        conn = ns.Connection(X, Y, w=w)
    else:
        tshape = target_shape(c)
        Y = ns.AdaptiveLIFNodes(shape=tshape, traces=True, rest=-65.0, reset=-60.0, thresh=-52.0, refrac=5, tc_trace=20.0,
                                theta_plus=0.05, tc_theta_decay=1e6)
        cls = {"lc1d": ns.LocalConnection1D, "lc2d": ns.LocalConnection2D, "lc3d": ns.LocalConnection3D}[c["kind"]]
        kw = dict(kernel_size=c["k"], stride=c["s"], n_filters=c["F"], nu=c["nu"], update_rule=ns.PostPre, wmin=0.0, wmax=1.0)
        if c["norm"] is not None:
            kw["norm"] = c["norm"]
        conn = cls(X, Y, **kw)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(conn, source="X", target="Y")
    if c.get("inh"):
        # examples/mnist/loc2d_mnist.py: every neuron inhibits the other filters' neurons of its own receptive field
        F, conv = c["F"], int(np.prod(target_shape(c)[1:]))
        w_inh = torch.zeros(F, conv, F, conv)
        for f in range(F):
            for o in range(conv):
                w_inh[f, o, :, o] = -c["inh"]
                w_inh[f, o, f, o] = 0
        net.add_connection(ns.Connection(Y, Y, w=w_inh.reshape(Y.n, Y.n)), source="Y", target="Y")
    if not c["train"]:
        net.train(False)
    return net


def inputs(name, r):
    """Input `r` of a case: [T, B, *input shape] uint8, from numpy's generator (same draws everywhere)."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c["seed"] + r + 7)
    return (rng.random((c["T"], c["B"], c["cin"], *c["shape"])) < c["density"]).astype(np.uint8)


def w_of(net):
    return net.connections[("X", "Y")].w


def snapshot(net, raster):
    X, Y = net.layers["X"], net.layers["Y"]
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).copy()
    return dict(raster=np.asarray(raster, np.uint8), v=f(Y.v), refrac=f(Y.refrac_count), theta=f(Y.theta), xX=f(X.x),
                xY=f(Y.x), w=f(w_of(net)))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(net, name, monitor_cls, device=None, first=0, count=None):
    """Run inputs [first, first+count) of the case (reset_state_variables() between them, as the example does); returns one
    snapshot per input."""
    c = CASES[name]
    out = []
    count = c["n_in"] - first if count is None else count
    for r in range(first, first + count):
        mon = monitor_cls(net.layers["Y"], ["s"], time=c["T"])
        net.add_monitor(mon, name="Y_s")
        x = torch.from_numpy(inputs(name, r))
        if device is not None:
            x = x.to(device)
        net.run({"X": x}, time=run_time(c["T"], c.get("dt", 1.0)))
        raster = mon.get("s").cpu().numpy().reshape(c["T"], c["B"], -1).astype(np.uint8)
        out.append(snapshot(net, raster))
        del net.monitors["Y_s"]
        net.reset_state_variables()
    return out
