"""The state-monitor fixture cases (tests/golden/make_golden_state_monitors.py), written once for both implementations: `build(ns,
name)` constructs a case's network from a namespace of classes -- the reference's (the generator) or this package's (the tests) --
and `run_case` drives it with two consecutive inputs (reset_state_variables() in between) and keeps, per input, everything the
case's monitors recorded, the layers' final state, the learned weights and the global generator's state.

Only families that reproduce the reference bit for bit: MulticompartmentConnection with a Weight (float32, or float16 in (h)) and
MCC PostPre, feeding DiehlAndCookNodes / CurrentLIFNodes / AdaptiveLIFNodes / LIFNodes.

  (a) Input 12 (traces) -> [Weight] + PostPre -> DiehlAndCookNodes 10, B = 3: x of both layers, theta, refrac_count, v, s of the target
  (b) -> CurrentLIFNodes 11, B = 2: i, x, refrac_count
  (every case also records the target's s, so that the generator can demand spikes of each)
  (c) -> AdaptiveLIFNodes 9 (odd: the slices of its [T, 9] theta recording are 4-byte aligned only), B = 2
  (d) (a) through NetworkMonitor(state_vars=("s", "v", "x", "theta"), time=T // 2)
  (e) (a) with one_step=True
  (f) (a) at dt = 0.5
  (g) activity: X -> Y through [Weight] + PostPre with traces=True and a recurrent Y -> Y [Probability, Weight] with traces=True --
      two contributions into one layer --, B = 2: both `activity`s and v
  (h) (g)'s first connection alone with a float16 Weight
"""
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time

LAYER_A = {"X": ("x",), "Y": ("x", "theta", "refrac_count", "v", "s")}
CASES = {
    "a": dict(target="dc", S=12, N=10, B=3, T=40, wscale=3.0, density=0.3, seed=71, layers=LAYER_A),
    "b": dict(target="clif", S=12, N=11, B=2, T=40, wscale=3.0, density=0.3, seed=72, layers={"Y": ("i", "x", "refrac_count", "s")}),
    "c": dict(target="alif", S=12, N=9, B=2, T=40, wscale=3.0, density=0.3, seed=73, layers={"Y": ("theta", "x", "refrac_count", "s")}),
    "d": dict(target="dc", S=12, N=10, B=3, T=40, wscale=3.0, density=0.3, seed=71, netmon=("s", "v", "x", "theta")),
    "e": dict(target="dc", S=12, N=10, B=3, T=40, wscale=3.0, density=0.3, seed=71, layers=LAYER_A, one_step=True),
    "f": dict(target="dc", S=12, N=10, B=3, T=40, wscale=3.0, density=0.3, seed=71, layers=LAYER_A, dt=0.5),
    "g": dict(target="lif", S=12, N=10, B=2, T=40, wscale=3.0, density=0.3, seed=74, layers={"Y": ("v", "s")}, traces=True, recurrent=True),
    "h": dict(target="lif", S=12, N=10, B=2, T=40, wscale=3.0, density=0.3, seed=75, layers={"Y": ("v", "s")}, traces=True, half=True),
}
STATE = ("v", "refrac_count", "x", "theta", "i")


def ns_from(nodes, topology, features, mcc_learning, network_cls, monitors):
    return SimpleNamespace(Input=nodes.Input, LIFNodes=nodes.LIFNodes, DiehlAndCookNodes=nodes.DiehlAndCookNodes,
                           CurrentLIFNodes=nodes.CurrentLIFNodes, AdaptiveLIFNodes=nodes.AdaptiveLIFNodes,
                           MulticompartmentConnection=topology.MulticompartmentConnection, Probability=features.Probability,
                           Weight=features.Weight, PostPre=mcc_learning.PostPre, Network=network_cls, Monitor=monitors.Monitor,
                           NetworkMonitor=monitors.NetworkMonitor)


def build(ns, name):
    c = CASES[name]
    S, N = c["S"], c["N"]
    rng = np.random.default_rng(c["seed"])                  # (values never touch torch's generator: the run alone consumes it)
    torch.manual_seed(c["seed"])
    net = ns.Network(dt=c.get("dt", 1.0), batch_size=c["B"])
    X = ns.Input(n=S, traces=True, tc_trace=20.0)
    cls = {"dc": ns.DiehlAndCookNodes, "clif": ns.CurrentLIFNodes, "alif": ns.AdaptiveLIFNodes, "lif": ns.LIFNodes}[c["target"]]
    Y = cls(n=N, traces=True, tc_trace=20.0)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    w = (rng.random((S, N), dtype=np.float32) * np.float32(c["wscale"])).astype(np.float32)
    value = torch.from_numpy(w)
    kw = dict(value_dtype=torch.float16) if c.get("half") else {}
    if c.get("half"):
        value = value.to(torch.float16)
    feat = ns.Weight("w_in", value, range=[0.0, float(c["wscale"])], nu=(1e-3, 1e-2), learning_rule=ns.PostPre, **kw)
    kw = dict(traces=True) if c.get("traces") else {}
    net.add_connection(ns.MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat], **kw), source="X", target="Y")
    feat.learning_rule.reduction = torch.sum                # (the constructor takes the default for batch size 1)
    if c.get("recurrent"):
        p = (0.5 + 0.5 * rng.random((N, N), dtype=np.float32)).astype(np.float32)
        wr = (rng.random((N, N), dtype=np.float32) * np.float32(0.6) - np.float32(0.45)).astype(np.float32)       # mostly inhibitory
        pipe = [ns.Probability("p_rec", torch.from_numpy(p)), ns.Weight("w_rec", torch.from_numpy(wr))]
        net.add_connection(ns.MulticompartmentConnection(Y, Y, device="cpu", pipeline=pipe, traces=True), source="Y", target="Y")
    return net


def inputs(name, r):
    """Input `r` of a case: u8 [T, B, S] Bernoulli spikes from numpy's generator."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c["seed"] + r + 3)
    return (rng.random((c["T"], c["B"], c["S"])) < c["density"]).astype(np.uint8)


def _np(t):
    t = t.detach().cpu()
    if t.is_sparse:
        t = t.to_dense()
    return t.numpy().copy()


def attach(ns, net, name):
    """The case's monitors, new for every input: {monitor name: monitor}."""
    c = CASES[name]
    T = c["T"]
    mons = {}
    if "netmon" in c:
        mons["net"] = ns.NetworkMonitor(net, state_vars=c["netmon"], time=T // 2)
    for lname, vars_ in c.get("layers", {}).items():
        mons["L_" + lname] = ns.Monitor(net.layers[lname], list(vars_), time=T)
    if c.get("traces"):
        for (src, dst), conn in net.connections.items():
            mons[f"C_{src}_{dst}"] = ns.Monitor(conn, ["activity"], time=T)
    for k, m in mons.items():
        net.add_monitor(m, name=k)
    return mons


def collect(net, name, mons):
    """{"rec_<layer>_<var>" / "act_<src>_<dst>" / "net_<layer>_<var>": recording, "<var>_<layer>": final state, "w_<src>_<dst>_<k>":
    feature value, "rng": generator state} as numpy; spikes as uint8, float16 values widened to float32 (exact)."""
    c = CASES[name]
    T, B = c["T"], c["B"]
    out = {}
    for lname, vars_ in c.get("layers", {}).items():
        for v in vars_:
            a = _np(mons["L_" + lname].get(v))
            out[f"rec_{lname}_{v}"] = a.astype(np.uint8) if v == "s" else a.astype(np.float32)
    if c.get("traces"):
        for (src, dst) in net.connections:
            out[f"act_{src}_{dst}"] = _np(mons[f"C_{src}_{dst}"].get("activity").float()).astype(np.float32).reshape(T, B, -1)
    if "netmon" in c:
        rec = mons["net"].get()
        for lname in net.layers:
            for v, t in rec[lname].items():
                out[f"net_{lname}_{v}"] = _np(t).astype(np.float32)
    for lname, layer in net.layers.items():
        for k in STATE:
            t = getattr(layer, k, None)
            if isinstance(t, torch.Tensor):
                out[f"{k}_{lname}"] = _np(t).astype(np.float32)
    for (src, dst), conn in net.connections.items():
        for k, f in enumerate(conn.pipeline):
            out[f"w_{src}_{dst}_{k}"] = _np(f.value.float()).astype(np.float32)
    out["rng"] = torch.get_rng_state().numpy().copy()
    return out


def run_case(ns, net, name, device=None, n_in=2):
    c = CASES[name]
    outs = []
    for r in range(n_in):
        mons = attach(ns, net, name)
        x = torch.from_numpy(inputs(name, r).copy())
        if device is not None:
            x = x.to(device)
        net.run({"X": x}, time=run_time(c["T"], c.get("dt", 1.0)), one_step=bool(c.get("one_step", False)))
        outs.append(collect(net, name, mons))
        for k in mons:
            del net.monitors[k]
        net.reset_state_variables()
    return outs
