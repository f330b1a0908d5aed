"""The Conv1dConnection / Conv3dConnection fixture cases (tests/golden/make_golden_conv_nd.py), written once for both
implementations: `build(ns, case)` constructs a case's network from a namespace of classes -- the reference's (the generator)
or this package's (the tests) -- and `run_case` drives it and records, after every input, the Y raster, v, refrac_count,
theta, both traces, w and the global generator's position (DiehlAndCookNodes' one-spike draws come from it).

(a) the conv1d_MNIST.py graph: Input [1, 784] -> Conv1dConnection (k 56, s 28, 25 filters, PostPre nu = (1e-4, 1e-2),
    wmax 1, norm 0.4*56) -> DiehlAndCookNodes [25, 27], with the -100 recurrent inhibition between filters at the same
    position; 3 inputs x 50 steps, batch 1
(b) conv1d with 2 input channels, padding 1, stride 2, batch 3, norm on (the raw-reshape view of the PostPre operand)
(c) (a) at batch 33 (batch sums beyond 32 terms)
(d) the conv3d_MNIST.py geometry: Input [1, 28, 28, 28] (a 2-D pattern repeated along depth) -> Conv3dConnection (k 16, s 4,
    12 filters, PostPre nu = (0, 1e-2), wmax 1, norm 0.4*16**3) -> DiehlAndCookNodes [12, 4, 4, 4] with the inhibition
(e) a small conv3d: padding 1, batch 2, nu = (0, 2e-2)
(f) (a) with network.train(False);  (g) (d) with network.train(False) and nu = (1e-4, 1e-2)"""
import hashlib
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time

CASES = {
    "a": dict(kind="c1", cin=1, shape=(784,), k=56, s=28, p=0, F=25, B=1, T=50, n_in=3, density=0.05, nu=(1e-4, 1e-2),
              wmin=None, norm=0.4 * 56, inh=100.0, train=True, seed=10),
    "b": dict(kind="c1", cin=2, shape=(60,), k=6, s=2, p=1, F=4, B=3, T=40, n_in=2, density=0.2, nu=(1e-2, 2e-2),
              wmin=0.0, norm=0.4 * 6, inh=0.0, train=True, seed=11),
    "c": dict(kind="c1", cin=1, shape=(784,), k=56, s=28, p=0, F=25, B=33, T=50, n_in=2, density=0.05, nu=(1e-4, 1e-2),
              wmin=None, norm=0.4 * 56, inh=100.0, train=True, seed=12),
    "d": dict(kind="c3", cin=1, shape=(28, 28, 28), k=16, s=4, p=0, F=12, B=1, T=50, n_in=3, density=0.03, nu=(0.0, 1e-2),
              wmin=None, norm=0.4 * 16 ** 3, inh=100.0, train=True, seed=13),
    "e": dict(kind="c3", cin=1, shape=(6, 6, 6), k=3, s=2, p=1, F=3, B=2, T=40, n_in=2, density=0.3, nu=(0.0, 2e-2),
              wmin=0.0, norm=None, inh=0.0, train=True, seed=14),
    "f": dict(kind="c1", cin=1, shape=(784,), k=56, s=28, p=0, F=25, B=1, T=50, n_in=3, density=0.05, nu=(1e-4, 1e-2),
              wmin=None, norm=0.4 * 56, inh=100.0, train=False, seed=10),
    "g": dict(kind="c3", cin=1, shape=(28, 28, 28), k=16, s=4, p=0, F=12, B=1, T=50, n_in=2, density=0.03, nu=(1e-4, 1e-2),
              wmin=None, norm=0.4 * 16 ** 3, inh=100.0, train=False, seed=13),
}
# (e) at dt = 0.5 (default 1.0; `time = T * dt` is run): the refractory countdown and the decays of v / theta / both traces behind the
# conv propagation and its PostPre.  DiehlAndCookNodes lets one neuron per sample fire in a step, so it takes 120 steps until ten of the
# 81 neurons have fired three times (B = 1: with two samples the file outgrows its sibling).  `sibling`: the dt = 1 case it repeats.
CASES["e_dt05"] = dict(CASES["e"], dt=0.5, T=120, B=1, sibling="e")
BIG = ("a", "c", "d", "f", "g")          # w recorded as a sha256 per input, the final array once (not for g: learning off)


def ns_from(nodes, topology, learning, network_cls):
    return SimpleNamespace(Input=nodes.Input, DiehlAndCookNodes=nodes.DiehlAndCookNodes, Connection=topology.Connection,
                           Conv1dConnection=topology.Conv1dConnection, Conv3dConnection=topology.Conv3dConnection,
                           PostPre=learning.PostPre, Network=network_cls)


def target_shape(c):
    conv = [int((n - c["k"] + 2 * c["p"]) / c["s"]) + 1 for n in c["shape"]]
    return [c["F"], *conv]


def build(ns, name):
    """The case's network (weights drawn from the global generator after torch.manual_seed(seed))."""
    c = CASES[name]
    torch.manual_seed(c["seed"])
    net = ns.Network(dt=c.get("dt", 1.0))
    X = ns.Input(shape=[c["cin"], *c["shape"]], traces=True)
    tshape = target_shape(c)
    Y = ns.DiehlAndCookNodes(shape=tshape, traces=True)
    cls = ns.Conv1dConnection if c["kind"] == "c1" else ns.Conv3dConnection
    kw = dict(kernel_size=c["k"], stride=c["s"], padding=c["p"], update_rule=ns.PostPre, nu=list(c["nu"]), wmax=1.0)
    if c["wmin"] is not None:
        kw["wmin"] = c["wmin"]
    if c["norm"] is not None:
        kw["norm"] = c["norm"]
    conn = cls(X, Y, **kw)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(conn, source="X", target="Y")
    if c["inh"]:
        # conv1d_MNIST.py / conv3d_MNIST.py: every neuron inhibits the other filters' neurons at its own position
        F, conv = c["F"], int(np.prod(tshape[1:]))
        w = torch.zeros(F, conv, F, conv)
        for f1 in range(F):
            for f2 in range(F):
                if f1 != f2:
                    w[f1, torch.arange(conv), f2, torch.arange(conv)] = -c["inh"]
        net.add_connection(ns.Connection(Y, Y, w=w.view(Y.n, Y.n)), source="Y", target="Y")
    if not c["train"]:
        net.train(False)
    return net


def inputs(name, r):
    """Input `r` of a case: [T, B, Cin, *shape] uint8 from numpy's generator; the conv3d cases repeat one 2-D pattern per step
    along depth, as conv3d_MNIST.py repeats the digit."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c["seed"] + r + 7)
    if c["kind"] == "c3" and c["shape"][0] == 28:
        plane = (rng.random((c["T"], c["B"], c["cin"], 1, *c["shape"][1:])) < c["density"]).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(plane, c["shape"][0], axis=3))
    return (rng.random((c["T"], c["B"], c["cin"], *c["shape"])) < c["density"]).astype(np.uint8)


def conn_of(net):
    return net.connections[("X", "Y")]


def generator_probe():
    """Four draws of the global generator, which is left where it was: pins its position after a run."""
    state = torch.get_rng_state()
    v = torch.rand(4).numpy().copy()
    torch.set_rng_state(state)
    return v


def snapshot(net, raster):
    X, Y = net.layers["X"], net.layers["Y"]
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).copy()       # noqa: E731
    return dict(raster=np.asarray(raster, np.uint8), v=f(Y.v), refrac=f(Y.refrac_count), theta=f(Y.theta), xX=f(X.x),
                xY=f(Y.x), w=f(conn_of(net).w), gen=generator_probe())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(net, name, monitor_cls, device=None, first=0, count=None):
    """Run inputs [first, first+count) of the case (reset_state_variables() between them, as the examples do); returns one
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
