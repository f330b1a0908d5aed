"""The MaxPool1d / 2d / 3dConnection and MeanFieldConnection fixture cases (tests/golden/make_golden_pool.py), written once for both
implementations: `build(ns, case)` constructs a case's network from a namespace of classes -- the reference's (the generator) or this
package's (the tests) -- and `run_case` drives it and records, after every input, the target raster, the target's state and the
pooling connection's `firing_rates` (case h: the convolution's learned `w` too).

Pooling cases: Input (C, *spatial) -> pool -> LIFNodes (C, *pooled), thresh -62.5 and refrac 1 (three pooled spikes in close succession cross it), 30 steps,
spike density 0.4, two consecutive inputs with reset_state_variables() between them.
(a) 2-D [2,6,6] k2 s2, B=3                        (b) 2-D [2,7,5] k(3,2) s(2,1) p(1,1): overlapping windows, padding
(c) 2-D [2,9,9] k3 s2 dilation 2                  (d) 1-D [3,11] k3 s2 p1
(e) 3-D [2,5,4,6] k(3,2,2) s(1,2,2) p1            (f) [1,5,5] k2 s1 at B=1: both leading dimensions are squeezed
(g1) (a) with decay=1.0 (what ann_to_snn passes: the rates ARE the last spikes)        (g0) (a) with decay=0.0 (spike counts)
(h) Input (1,10,10) -> Conv2dConnection (4 filters 3x3, PostPre) -> LIF (4,8,8) -> MaxPool2dConnection(2, 2) -> IFNodes (4,4,4)
    with a recurrent MeanFieldConnection(w=-0.5) on the IF layer, network.train(True), B=2
Mean-field cases: Input 50 -> MeanFieldConnection -> LIF 20, B=2:
(m1) 0-dim w   (m2) w of shape [20]   (m3) no w given: the constructor's draw between wmin=2 and wmax=40"""
import hashlib
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time

POOL = {
    "a": dict(nd=2, shape=(2, 6, 6), k=2, s=2, p=0, d=1, B=3, decay=0.2),
    "b": dict(nd=2, shape=(2, 7, 5), k=(3, 2), s=(2, 1), p=(1, 1), d=1, B=2, decay=0.2),
    "c": dict(nd=2, shape=(2, 9, 9), k=3, s=2, p=0, d=2, B=2, decay=0.3),
    "d": dict(nd=1, shape=(3, 11), k=3, s=2, p=1, d=1, B=2, decay=0.2),
    "e": dict(nd=3, shape=(2, 5, 4, 6), k=(3, 2, 2), s=(1, 2, 2), p=1, d=1, B=2, decay=0.25),
    "f": dict(nd=2, shape=(1, 5, 5), k=2, s=1, p=0, d=1, B=1, decay=0.2),
    "g1": dict(nd=2, shape=(2, 6, 6), k=2, s=2, p=0, d=1, B=3, decay=1.0),
    "g0": dict(nd=2, shape=(2, 6, 6), k=2, s=2, p=0, d=1, B=3, decay=0.0),
}
MEAN = {
    "m1": dict(w=lambda: torch.tensor(3.0), kw={}),
    "m2": dict(w=lambda: 4.0 * torch.rand(20, generator=torch.Generator().manual_seed(77)), kw={}),
    "m3": dict(w=None, kw=dict(wmin=2.0, wmax=40.0)),
}
# (h) -- the case with a learning rule -- at dt = 0.5 (`time = T * dt` is run): the refractory countdown (1 and 2 ms: two and four
# steps) and the decays of both node layers and their traces.  A dt case is its sibling (the name before "_dt") at another timestep, with
# the sibling's seed and input; listed last, so that seed_of() of the others stays.
DT = {"h_dt05": dict(dt=0.5, rate=0.3, T=30, B=1)}     # (at the others' input rate of 0.4 the rule empties the weights and the second input is silent; B = 1 keeps the file under its sibling's size)
CASES = sorted(POOL) + ["h"] + sorted(MEAN) + sorted(DT)
T, N_IN, RATE = 30, 2, 0.4
H = dict(shape=(1, 10, 10), filters=4, k=3, B=2, seed=58)


def base(name):
    return name.split("_dt")[0]


def dt_of(name):
    return DT[name]["dt"] if name in DT else 1.0


def steps_of(name):
    return DT[name]["T"] if name in DT else T


def seed_of(name):
    return 300 + CASES.index(base(name))


def batch_of(name):
    return POOL[name]["B"] if name in POOL else DT[name]["B"] if name in DT else 2


def ns_from(nodes, topology, network_cls, learning):
    return SimpleNamespace(Input=nodes.Input, LIFNodes=nodes.LIFNodes, IFNodes=nodes.IFNodes, Network=network_cls, PostPre=learning.PostPre,
                           Conv2dConnection=topology.Conv2dConnection, MeanFieldConnection=topology.MeanFieldConnection,
                           pool={1: topology.MaxPool1dConnection, 2: topology.MaxPool2dConnection, 3: topology.MaxPoo3dConnection})


def tup(v, nd):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * nd


def pooled_shape(c):
    nd = c["nd"]
    out = [(i + 2 * p - d * (k - 1) - 1) // s + 1
           for i, k, s, p, d in zip(c["shape"][1:], tup(c["k"], nd), tup(c["s"], nd), tup(c["p"], nd), tup(c["d"], nd))]
    return (c["shape"][0], *out)


def window_taps(c):
    """int array [O, K]: for every pooled position of one plane (row-major) the flat plane indices of its in-bounds taps in row-major
    scan order, packed to the front and padded with -1.  Written from the pooling definition alone (no torch), so that the index rule
    can be checked against it."""
    nd = c["nd"]
    spatial = c["shape"][1:]
    ks, ss, ps, ds = (tup(c[key], nd) for key in ("k", "s", "p", "d"))
    out = pooled_shape(c)[1:]
    K = int(np.prod(ks))
    rows = []
    for o in np.ndindex(*out):
        taps = []
        for kk in np.ndindex(*ks):
            pos = [o[a] * ss[a] - ps[a] + kk[a] * ds[a] for a in range(nd)]
            if all(0 <= pos[a] < spatial[a] for a in range(nd)):
                taps.append(int(np.ravel_multi_index(pos, spatial)))
        rows.append(taps + [-1] * (K - len(taps)))
    return np.asarray(rows, np.int64)


def window_stats(fr, taps):
    """(first-maximum indices [B, C, O], how many windows picked a tap other than their first in-bounds one, how many hold their
    maximum more than once, windows in all) for rates fr [B, C, *spatial] (finite values)."""
    B, C = fr.shape[:2]
    flat = np.asarray(fr, np.float32).reshape(B, C, -1)
    vals = np.where(taps >= 0, flat[:, :, np.maximum(taps, 0)], -np.inf)           # [B, C, O, K]
    arg = vals.argmax(-1)                                                           # numpy: the first maximum
    idx = np.take_along_axis(np.broadcast_to(taps, vals.shape), arg[..., None], -1)[..., 0]
    ties = (vals == vals.max(-1, keepdims=True)).sum(-1) > 1
    return idx, int((arg != 0).sum()), int(ties.sum()), int(arg.size)


def build(ns, name):
    torch.manual_seed(seed_of(name))
    if name in POOL:
        c = POOL[name]
        net = ns.Network(dt=1.0, batch_size=c["B"])
        net.add_layer(ns.Input(shape=c["shape"], traces=True), name="X")
        net.add_layer(ns.LIFNodes(shape=pooled_shape(c), traces=True, thresh=-62.5, refrac=1), name="Y")
        conn = ns.pool[c["nd"]](net.layers["X"], net.layers["Y"], kernel_size=c["k"], stride=c["s"], padding=c["p"], dilation=c["d"],
                                decay=c["decay"])
        net.add_connection(conn, source="X", target="Y")
        net.train(False)                            # (the reference's pooling classes run in eval mode only)
        return net
    if base(name) == "h":
        net = ns.Network(dt=dt_of(name), batch_size=batch_of(name))
        F, k = H["filters"], H["k"]
        side = H["shape"][1] - k + 1
        net.add_layer(ns.Input(shape=H["shape"], traces=True), name="X")
        net.add_layer(ns.LIFNodes(shape=(F, side, side), traces=True, thresh=-64.0, refrac=1), name="C")
        net.add_layer(ns.IFNodes(shape=(F, side // 2, side // 2), traces=True, thresh=-63.0, refrac=2), name="Y")
        net.add_connection(ns.Conv2dConnection(net.layers["X"], net.layers["C"], kernel_size=k, stride=1, update_rule=ns.PostPre,
                                               nu=(1e-2, 2e-2), reduction=torch.sum, wmin=0.0, wmax=1.0), source="X", target="C")
        net.add_connection(ns.pool[2](net.layers["C"], net.layers["Y"], kernel_size=2, stride=2, decay=0.2), source="C", target="Y")
        net.add_connection(ns.MeanFieldConnection(net.layers["Y"], net.layers["Y"], w=torch.tensor(-0.5)), source="Y", target="Y")
        net.train(True)
        return net
    m = MEAN[name]
    net = ns.Network(dt=1.0, batch_size=2)
    net.add_layer(ns.Input(n=50, traces=True), name="X")
    net.add_layer(ns.LIFNodes(n=20, traces=True, thresh=-60.0, refrac=1), name="Y")
    kw = dict(m["kw"])
    if m["w"] is not None:
        kw["w"] = m["w"]()
    net.add_connection(ns.MeanFieldConnection(net.layers["X"], net.layers["Y"], **kw), source="X", target="Y")
    net.train(False)
    return net


def pool_of(net):
    """The network's pooling connection, or None."""
    for conn in net.connections.values():
        if hasattr(conn, "firing_rates"):
            return conn
    return None


def inputs(name, r):
    """Input `r` of a case: [T, B, *shape] uint8 from numpy's generator."""
    shape = POOL[name]["shape"] if name in POOL else H["shape"] if base(name) == "h" else (50,)
    rng = np.random.default_rng(1000 * seed_of(name) + r)
    return (rng.random((steps_of(name), batch_of(name), *shape)) < (DT[name]["rate"] if name in DT else RATE)).astype(np.uint8)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def snapshot(net, raster):
    Y = net.layers["Y"]
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).copy()       # noqa: E731
    out = dict(raster=np.asarray(raster, np.uint8), v=f(Y.v), refrac=f(Y.refrac_count), xY=f(Y.x))
    pool = pool_of(net)
    if pool is not None:
        out["fr"] = f(pool.firing_rates)
    for key, conn in net.connections.items():
        if key == ("X", "C"):
            out["w"] = f(conn.w)
    return out


def run_case(net, name, monitor_cls, device=None, first=0, count=None, split=False):
    """Run inputs [first, first+count) of the case (reset_state_variables() between them); one snapshot per input.  split: every
    input is run as two halves, with one monitor over both."""
    out = []
    count = N_IN - first if count is None else count
    dt, T = dt_of(name), steps_of(name)
    for r in range(first, first + count):
        mon = monitor_cls(net.layers["Y"], ["s"], time=T)
        net.add_monitor(mon, name="Y_s")
        x = torch.from_numpy(inputs(name, r))
        if device is not None:
            x = x.to(device)
        if split:
            net.run({"X": x[:T // 2].clone()}, time=run_time(T // 2, dt))
            net.run({"X": x[T // 2:].clone()}, time=run_time(T - T // 2, dt))
        else:
            net.run({"X": x}, time=run_time(T, dt))
        raster = mon.get("s").cpu().numpy().reshape(T, batch_of(name), -1).astype(np.uint8)
        out.append(snapshot(net, raster))
        del net.monitors["Y_s"]
        net.reset_state_variables()
    return out


# ---- constructors and raising calls --------------------------------------------------------------------------------------------

def generator_probe():
    """Four draws of the global generator, which is left where it was: pins its position."""
    state = torch.get_rng_state()
    v = torch.rand(4).numpy().copy()
    torch.set_rng_state(state)
    return v


CTOR = {
    "default": dict(),
    "bounded": dict(wmin=-1.0, wmax=2.0),
    "wmax_only": dict(wmax=0.05),
    "given": dict(w=torch.tensor(0.7)),
    "given_bounded": dict(w=torch.tensor(5.0), wmin=0.0, wmax=1.0),           # finite bounds: NOT clamped (topology.py:1967)
    "given_half_bounded": dict(w=torch.tensor([5.0, -3.0, 0.2]), wmax=1.0),   # an infinite bound: clamped
    "weight_decay": dict(weight_decay=0.5),                                   # lands in the `reduction` slot
}


def ctor(ns, variant):
    """One MeanFieldConnection constructor variant after torch.manual_seed(9): (connection, generator probe behind it)."""
    torch.manual_seed(9)
    kw = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in CTOR[variant].items()}
    conn = ns.MeanFieldConnection(ns.Input(n=6), ns.LIFNodes(n=3), **kw)
    return conn, generator_probe()


def _pool_net(ns, shape, B, decay=0.2, before=False, target=None):
    net = ns.Network(dt=1.0, batch_size=B)
    X = ns.Input(shape=shape, traces=True)
    c = dict(nd=2, shape=shape, k=2, s=2, p=0, d=1)
    Y = ns.LIFNodes(shape=pooled_shape(c) if target is None else target, traces=True)
    kw = {} if decay is None else dict(decay=decay)
    if before:
        conn = ns.pool[2](X, Y, kernel_size=2, stride=2, **kw)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    if not before:
        conn = ns.pool[2](X, Y, kernel_size=2, stride=2, **kw)
    net.add_connection(conn, source="X", target="Y")
    net.train(False)
    return net


def _run_pool(net, shape, B, steps=3):
    x = (np.random.default_rng(5).random((steps, B, *shape)) < 0.5).astype(np.uint8)
    net.run({"X": torch.from_numpy(x)}, time=steps)
    return net


def _mean_net(ns, **kw):
    net = ns.Network(dt=1.0, batch_size=2)
    net.add_layer(ns.Input(n=6, traces=True), name="X")
    net.add_layer(ns.LIFNodes(n=3, traces=True), name="Y")
    net.add_connection(ns.MeanFieldConnection(net.layers["X"], net.layers["Y"], **kw), source="X", target="Y")
    net.train(False)
    return net


def _run_mean(net):
    net.run({"X": torch.ones(3, 2, 6, dtype=torch.uint8)}, time=3)
    return net


def _train(net):
    net.train(True)
    return net


# name -> a call that takes the class namespace; the generator records what each does in the reference ("ok" or the exception's name)
CALLS = {
    "pool_decay_none": lambda ns: _run_pool(_pool_net(ns, (2, 4, 4), 2, decay=None), (2, 4, 4), 2),
    "pool_b1": lambda ns: _run_pool(_pool_net(ns, (2, 4, 4), 1), (2, 4, 4), 1),
    "pool_b1_c1": lambda ns: _run_pool(_pool_net(ns, (1, 4, 4), 1), (1, 4, 4), 1),
    "pool_b2_c1": lambda ns: _run_pool(_pool_net(ns, (1, 4, 4), 2), (1, 4, 4), 2),
    "pool_inner_one": lambda ns: _run_pool(_pool_net(ns, (2, 1, 4), 2, target=(2, 1, 2)), (2, 1, 4), 2),
    "pool_target_shape": lambda ns: _run_pool(_pool_net(ns, (2, 4, 4), 2, target=(8,)), (2, 4, 4), 2),
    "pool_built_before_layers": lambda ns: _run_pool(_pool_net(ns, (2, 4, 4), 2, before=True), (2, 4, 4), 2),
    "pool_training_mode": lambda ns: _run_pool(_train(_pool_net(ns, (2, 4, 4), 2)), (2, 4, 4), 2),
    "pool_other_batch_without_reset": lambda ns: _run_pool(_pool_net(ns, (2, 4, 4), 2), (2, 4, 4), 3),
    "mean_postpre": lambda ns: _mean_net(ns, update_rule=ns.PostPre, nu=1e-2),
    "mean_norm": lambda ns: _run_mean(_mean_net(ns, w=0.5 * torch.ones(3), norm=1.0)),
    "mean_training_mode": lambda ns: _run_mean(_train(_mean_net(ns, w=torch.tensor(0.5)))),
    "mean_weight_decay_training": lambda ns: _run_mean(_train(_mean_net(ns, w=torch.tensor(0.5), weight_decay=0.5))),
    "mean_recurrent_inhibition": lambda ns: _run_pool(_recurrent(ns), (2, 4, 4), 2),
}


def _recurrent(ns):
    net = _pool_net(ns, (2, 4, 4), 2)
    net.add_connection(ns.MeanFieldConnection(net.layers["Y"], net.layers["Y"], w=torch.tensor(-0.5)), source="Y", target="Y")
    return net


def outcome(ns, call):
    try:
        CALLS[call](ns)
    except Exception as e:         # noqa: BLE001  (the point is to record which)
        return type(e).__name__
    return "ok"
