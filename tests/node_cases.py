"""The node-layer fixture cases (tests/golden/make_golden_nodes.py), written once for both implementations: `build(ns, case)`
constructs a case's network from a namespace of classes -- the reference's (the generator) or this package's (the tests) --
and `run_case` drives it and records, per input, the Y raster, the per-step v record and every final state tensor.

direct cases   layer Y alone, driven by run(inputs={"Y": current}) with an f32 [T, B, n] external current: node arithmetic
               without propagation.  B in {1, 4}, with / without lbound, refrac 0 / 5, additive / non-additive traces.
mcc cases      Input(traces=True) -> MulticompartmentConnection + Weight with PostPre -> layer Y: the rule reads the new
               layers' `s` and `x`.
izh cases      IzhikevichNodes n = 100 at excitatory = 1, 0 and 0.8, B = 1 and 4; r, a, b, c, d, S come from the fixture, so run
               parity does not depend on constructor parity (CTOR pins the constructor on its own).
"""
import hashlib
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time, tag

KINDS = ("mcp", "if", "boosted", "clif", "izh")

# per kind: constructor arguments that stay fixed, and the range [lo, hi) the uniform external current is drawn from
_DIRECT = {
    "mcp": (dict(thresh=1.0), (-0.5, 1.5)),
    "if": (dict(thresh=-52.0, reset=-65.0), (-2.0, 5.0)),
    "boosted": (dict(thresh=13.0, tc_decay=100.0), (-1.0, 5.0)),
    "clif": (dict(thresh=-52.0, rest=-65.0, reset=-65.0, tc_decay=100.0, tc_i_decay=2.0), (-0.5, 2.0)),
}

CASES = {}
for kind in ("mcp", "if", "boosted", "clif"):
    CASES[f"{kind}_b1"] = dict(kind=kind, graph="direct", n=48, B=1, T=50, n_in=2, refrac=5, lbound=None, additive=False, seed=11)
    CASES[f"{kind}_b4"] = dict(kind=kind, graph="direct", n=37, B=4, T=50, n_in=3, refrac=0, lbound=True, additive=True, seed=12)
    CASES[f"{kind}_mcc"] = dict(kind=kind, graph="mcc", n=20, n_src=40, B=2, T=50, n_in=2, refrac=5, lbound=None, additive=False,
                                seed=13, density=0.25)
CASES["izh_e1_b1"] = dict(kind="izh", graph="direct", n=100, B=1, T=60, n_in=2, exc=1, lbound=None, additive=False, seed=21)
CASES["izh_e0_b4"] = dict(kind="izh", graph="direct", n=100, B=4, T=60, n_in=2, exc=0, lbound=True, additive=True, seed=22)
CASES["izh_mix_b1"] = dict(kind="izh", graph="direct", n=100, B=1, T=60, n_in=3, exc=0.8, lbound=True, additive=False, seed=23)
CASES["izh_mix_b4"] = dict(kind="izh", graph="direct", n=100, B=4, T=60, n_in=2, exc=0.8, lbound=None, additive=True, seed=24)
CASES["izh_mcc"] = dict(kind="izh", graph="mcc", n=20, n_src=40, B=2, T=50, n_in=2, exc=0.8, lbound=None, additive=False, seed=25,
                        density=0.25)


# dt != 1 (default 1.0): `time = T * dt` is run, so T stays the step count.  The refractory counter is `rc -= dt`, every decay
# exp(-dt / tc), Izhikevich steps by dt / 2 twice and MCC PostPre multiplies by dt.  refrac 5 at dt 2.0 counts 5, 3, 1, -1 (no
# multiple); refrac 1.0 at dt 0.1 is ten f32 subtractions of 0.1f.  0.5 and 2.0 scale exactly in f32, 0.1 and 0.3 do not.
for kind in ("if", "boosted", "clif"):
    for dt, refrac, T in ((0.5, 5, 80), (2.0, 5, 50), (0.1, 1.0, 120)):
        CASES[f"{kind}_b4_{tag(dt)}"] = dict(kind=kind, graph="direct", n=37, B=4, T=T, n_in=2, refrac=refrac, lbound=True, additive=True,
                                             seed=12, dt=dt, sibling=f"{kind}_b4")
CASES["mcp_b4_dt05"] = dict(kind="mcp", graph="direct", n=37, B=4, T=50, n_in=2, refrac=0, lbound=True, additive=True, seed=12, dt=0.5,
                            sibling="mcp_b4")
CASES["izh_mix_b4_dt05"] = dict(kind="izh", graph="direct", n=100, B=4, T=60, n_in=2, exc=0.8, lbound=None, additive=True, seed=24, dt=0.5,
                                sibling="izh_mix_b4")
CASES["izh_e0_b1_dt03"] = dict(kind="izh", graph="direct", n=100, B=1, T=120, n_in=2, exc=0, lbound=True, additive=True, seed=22, dt=0.3,
                               sibling="izh_e0_b4")
CASES["if_mcc_dt03"] = dict(kind="if", graph="mcc", n=20, n_src=40, B=2, T=50, n_in=2, refrac=5, lbound=None, additive=False, seed=13,
                            density=0.25, dt=0.3, sibling="if_mcc")
CASES["izh_mcc_dt03"] = dict(kind="izh", graph="mcc", n=20, n_src=40, B=2, T=40, n_in=2, exc=0.8, lbound=None, additive=False, seed=25,
                             density=0.25, dt=0.3, sibling="izh_mcc")

LBOUND = {"if": -66.0, "clif": -65.25, "izh": -70.0}          # (McCullochPitts and BoostedLIFNodes have none)
IZH_RANGE = {1: (0.0, 9.0), 0: (0.0, 30.0), 0.8: (0.0, 12.0)}  # external current per excitatory regime
STATE = ("v", "refrac_count", "i", "u", "x")                   # what a layer may have; stored where it does

# the constructor case: (seed, n, excitatory) -- every regime, and the clamped out-of-range values
CTOR = [(5, 10, 1), (6, 10, 0), (7, 10, 0.8), (8, 33, 0.5), (9, 7, 1.5), (10, 7, -1)]
IZH_BUFFERS = ("r", "a", "b", "c", "d", "S", "excitatory")


def ns_from(nodes, topology, features, mcc_learning, network_cls):
    return SimpleNamespace(Input=nodes.Input, McCullochPitts=nodes.McCullochPitts, IFNodes=nodes.IFNodes,
                           BoostedLIFNodes=nodes.BoostedLIFNodes, CurrentLIFNodes=nodes.CurrentLIFNodes,
                           IzhikevichNodes=nodes.IzhikevichNodes, MulticompartmentConnection=topology.MulticompartmentConnection,
                           Weight=features.Weight, PostPre=mcc_learning.PostPre, Network=network_cls)


def make_layer(ns, c, izh=None):
    """The case's layer Y.  izh: {r, a, b, c, d, S, excitatory} arrays loaded into an IzhikevichNodes after construction."""
    kind = c["kind"]
    kw = dict(n=c["n"], traces=True, traces_additive=c["additive"], tc_trace=20.0)
    if c["lbound"] and kind in LBOUND:
        kw["lbound"] = LBOUND[kind]
    if kind == "izh":
        Y = ns.IzhikevichNodes(excitatory=c["exc"], **kw)
        if izh is not None:
            for name in IZH_BUFFERS:
                setattr(Y, name, torch.from_numpy(np.array(izh[name])))
        return Y
    kw.update(_DIRECT[kind][0])
    if kind != "mcp":
        kw["refrac"] = c["refrac"]
    cls = {"mcp": ns.McCullochPitts, "if": ns.IFNodes, "boosted": ns.BoostedLIFNodes, "clif": ns.CurrentLIFNodes}[kind]
    return cls(**kw)


def mcc_scale(c):
    """Weights of the mcc cases are uniform in [0, scale): the summed current makes the layer spike at a moderate rate."""
    return {"mcp": 0.13, "if": 1.0, "boosted": 1.0, "clif": 0.5, "izh": 3.0}[c["kind"]]


def build(ns, name, izh=None):
    c = CASES[name]
    torch.manual_seed(c["seed"])
    net = ns.Network(dt=c.get("dt", 1.0))
    Y = make_layer(ns, c, izh)
    if c["graph"] == "mcc":
        X = ns.Input(n=c["n_src"], traces=True, tc_trace=20.0)
        w = np.random.default_rng(c["seed"]).random((c["n_src"], c["n"]), dtype=np.float32) * np.float32(mcc_scale(c))
        feat = ns.Weight("weight", torch.from_numpy(w), range=[0.0, float(mcc_scale(c))], nu=(1e-3, 1e-2), learning_rule=ns.PostPre)
        conn = ns.MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat])
        net.add_layer(X, name="X")
        net.add_layer(Y, name="Y")
        net.add_connection(conn, source="X", target="Y")
    else:
        net.add_layer(Y, name="Y")
    return net


def inputs(name, r):
    """Input `r` of a case, from numpy's generator: {"Y": f32 [T, B, n] current} or {"X": u8 [T, B, n_src] spikes}."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c["seed"] + r + 3)
    if c["graph"] == "mcc":
        return {"X": (rng.random((c["T"], c["B"], c["n_src"])) < c["density"]).astype(np.uint8)}
    lo, hi = IZH_RANGE[c["exc"]] if c["kind"] == "izh" else _DIRECT[c["kind"]][1]
    return {"Y": (lo + (hi - lo) * rng.random((c["T"], c["B"], c["n"]), dtype=np.float32)).astype(np.float32)}


def weights(net):
    conn = net.connections.get(("X", "Y"))
    return None if conn is None else conn.pipeline[0].value


def snapshot(net, raster, vrec):
    Y = net.layers["Y"]
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).copy()      # noqa: E731
    out = dict(raster=np.asarray(raster, np.uint8), vrec=np.asarray(vrec, np.float32))
    for k in STATE:
        t = getattr(Y, k, None)
        if isinstance(t, torch.Tensor):
            out[k] = f(t)
    if "X" in net.layers:
        out["xX"] = f(net.layers["X"].x)
        out["w"] = f(weights(net))
    return out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(net, name, monitor_cls, device=None, first=0, count=None, halves=False):
    """Run inputs [first, first+count) of the case (reset_state_variables() between them); one snapshot per input.
    halves: every input as two run() calls of T/2 steps.  A run of T steps lasts `T * dt`."""
    c = CASES[name]
    out = []
    T, dt = c["T"], c.get("dt", 1.0)
    count = c["n_in"] - first if count is None else count
    for r in range(first, first + count):
        mon = monitor_cls(net.layers["Y"], ["s", "v"], time=T)
        net.add_monitor(mon, name="Y_mon")
        inp = {k: torch.from_numpy(v.copy()) for k, v in inputs(name, r).items()}
        if device is not None:
            inp = {k: v.to(device) for k, v in inp.items()}
        if halves:
            net.run({k: v[:T // 2] for k, v in inp.items()}, time=run_time(T // 2, dt))
            net.run({k: v[T // 2:] for k, v in inp.items()}, time=run_time(T - T // 2, dt))
        else:
            net.run(inp, time=run_time(T, dt))
        raster = mon.get("s").cpu().numpy().reshape(T, c["B"], -1).astype(np.uint8)
        vrec = mon.get("v").cpu().numpy().reshape(T, c["B"], -1).astype(np.float32)
        out.append(snapshot(net, raster, vrec))
        del net.monitors["Y_mon"]
        net.reset_state_variables()
    return out


def breakout_graph(nodes, topology, learning, network_cls, hidden="izh", seed=0, fixed_grid=False):
    """The graph shape of the reference's examples/breakout/breakout.py with a reward-modulated rule on both connections:
    Input 6400 (traces) -> Connection (MSTDP) -> 100 hidden -> Connection (MSTDP) -> 4 output neurons, weights in [0, 1].
    hidden: "izh" (IzhikevichNodes, as in the example) or "lif" (LIFNodes: the same graph from layers every version has).
    fixed_grid: the same graph without the rule and with the weights rounded to multiples of 1/128: every partial sum of a dense product
    of spikes with them is exact in f32, so the currents do not depend on the order in which a BLAS or a kernel adds them."""
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    net = network_cls(dt=1.0)
    X = nodes.Input(n=6400, traces=True)
    if hidden == "izh":
        M, O = nodes.IzhikevichNodes(n=100, traces=True), nodes.IzhikevichNodes(n=4, traces=True)
        scale = (0.1, 1.0)
    else:
        M, O = nodes.LIFNodes(n=100, traces=True), nodes.LIFNodes(n=4, traces=True)
        scale = (0.05, 1.0)
    net.add_layer(X, name="X")
    net.add_layer(M, name="M")
    net.add_layer(O, name="O")
    for (src, dst), sc in zip((("X", "M"), ("M", "O")), scale):
        a, b = net.layers[src], net.layers[dst]
        w = torch.from_numpy(rng.random((a.n, b.n), dtype=np.float32) * np.float32(sc))
        if fixed_grid:
            w = torch.round(w * 128.0) / 128.0
            net.add_connection(topology.Connection(a, b, w=w, wmin=0.0, wmax=1.0), source=src, target=dst)
            continue
        net.add_connection(topology.Connection(a, b, w=w, wmin=0.0, wmax=1.0, update_rule=learning.MSTDP, nu=1e-3, reduction=torch.sum), source=src, target=dst)
    return net


def breakout_input(T, B, seed=0, p=0.02):
    """Bernoulli spikes [T, B, 6400] u8 at rate p."""
    return (np.random.default_rng(1000 + seed).random((T, B, 6400)) < p).astype(np.uint8)
