"""The per-timestep normalisation fixture cases (tests/golden/make_golden_norm_step.py), written once for both implementations:
`build(ns, case)` constructs a case's network from a namespace of classes -- the reference's (the generator) or this package's (the
tests) -- and `run` drives it with two inputs (reset_state_variables() between them) and records, per input, every layer's raster,
v, theta, refrac_count and trace, every feature value, the rule state of every Weight and the global generator's state.

Every Weight has norm_frequency="time step": the reference's Weight.compute normalises it behind the product that read it, once per
connection and timestep, learning or not (topology_features.py:633-645, :663-671).

(a) Input 40 -> Weight (0.3 * rand, range [0, 1], norm 4.0, PostPre nu = (1e-2, 2e-2)) -> DiehlAndCookNodes 12 (thresh -60,
    theta_plus 0.05), B = 3, 30 steps at 30 % density
(b) B = 1, MSTDP with reward 0.7 then -0.4, LIF target, one norm per target neuron (a tensor)
(c) NoOp with network.train(False): the column sums equal the norm after step 1 -- normalisation is not gated on learning
(d) [Probability, Weight] at B = 1: the Bernoulli draws of the global generator
(e) 70 x 37: columns on both sides of 32 * floor(N / 32); range [-1, 1] with negative weights, one all-zero column (the zero guard)
    and one column that sums to exactly 0 (+0.5 and -0.5)
(f) PostPre with average_update = 3
(g) one_step=True on a two-layer graph, both connections normalised every step
(h) (a) at dt = 0.5
(i) two such connections into one layer (the second accumulates onto the first)
(j) MSTDPET at B = 1"""
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time

INPUTS = 2
A_PLUS, A_MINUS = 1.0, -0.6
CASES = {
    "a": dict(S=40, N=12, B=3, T=30, density=0.3, rule="PostPre", target="dc", norm=4.0, seed=71),
    "b": dict(S=40, N=12, B=1, T=30, density=0.3, rule="MSTDP", target="lif", norm="vec", seed=72, rewards=(0.7, -0.4)),
    "c": dict(S=40, N=12, B=3, T=30, density=0.3, rule=None, target="dc", norm=4.0, seed=73, train=False),
    "d": dict(S=40, N=12, B=1, T=30, density=0.3, rule="PostPre", target="lif", norm=6.0, seed=74, pipe="PW"),
    "e": dict(S=70, N=37, B=3, T=30, density=0.3, rule="PostPre", target="lif", norm=8.0, seed=75, signed=True),
    "f": dict(S=40, N=12, B=3, T=30, density=0.3, rule="PostPre", target="dc", norm=4.0, seed=76, average_update=3),
    "g": dict(S=40, N=12, B=2, T=30, density=0.3, rule="PostPre", target="lif", norm=2.5, seed=77, graph="two_layer", one_step=True),
    "h": dict(S=40, N=12, B=3, T=30, density=0.3, rule="PostPre", target="dc", norm=4.0, seed=71, dt=0.5, sibling="a"),
    "i": dict(S=40, N=12, B=2, T=30, density=0.3, rule="PostPre", target="lif", norm=2.0, seed=79, graph="two_inputs"),
    "j": dict(S=40, N=12, B=1, T=30, density=0.3, rule="MSTDPET", target="lif", norm=5.0, seed=80, rewards=(0.7, -0.4)),
}
_NU = {"PostPre": (1e-2, 2e-2), "MSTDP": (1e-2, 0.0), "MSTDPET": (0.02, 0.0)}
RINGS = ("average_buffer_pre", "average_buffer_post", "average_buffer")
INDICES = ("average_buffer_index_pre", "average_buffer_index_post", "average_buffer_index")
STATE = ("p_plus", "p_minus", "eligibility_trace")


def ns_from(nodes, topology, features, mcc_learning, network_cls, monitor_cls):
    return SimpleNamespace(Input=nodes.Input, LIFNodes=nodes.LIFNodes, DiehlAndCookNodes=nodes.DiehlAndCookNodes,
                           MulticompartmentConnection=topology.MulticompartmentConnection, Weight=features.Weight,
                           Probability=features.Probability, mcc=mcc_learning, Network=network_cls, Monitor=monitor_cls)


def w0(case, tag, S, N):
    """The initial weights of connection `tag`, from numpy's generator (the torch generator is consumed by the run alone)."""
    c = CASES[case]
    rng = np.random.default_rng(c["seed"] * 100 + sum(map(ord, tag)))
    if c.get("signed"):
        w = (rng.random((S, N), dtype=np.float32) * np.float32(1.2) - np.float32(0.3)).astype(np.float32)
        w[:, 5] = 0.0                                  # an all-zero column: its sum is 0, the guard makes it 1
        w[:, 33] = 0.0                                 # a column that sums to exactly 0 in any order
        w[3, 33], w[40, 33] = 0.5, -0.5
        return np.clip(w, -1.0, 1.0)
    return (np.float32(0.3) * rng.random((S, N), dtype=np.float32)).astype(np.float32)


def norm_of(case, N):
    c = CASES[case]
    if c["norm"] == "vec":
        return torch.from_numpy(np.linspace(3.0, 5.0, N).astype(np.float32))
    return c["norm"]


def _target(ns, c, n):
    if c["target"] == "dc":
        return ns.DiehlAndCookNodes(n=n, traces=True, thresh=-60.0, theta_plus=0.05)
    return ns.LIFNodes(n=n, traces=True, tc_trace=20.0, thresh=-60.0, rest=-65.0, reset=-65.0, refrac=2, tc_decay=100.0)


def _connection(ns, case, tag, src, dst, frequency, norm=True):
    c = CASES[case]
    S, N = src.n, dst.n
    kw = {}
    if c["rule"] is not None:
        kw = dict(nu=list(_NU[c["rule"]]), learning_rule=getattr(ns.mcc, c["rule"]))
    feat = ns.Weight(f"weight_{tag}", torch.from_numpy(w0(case, tag, S, N)), range=[-1.0, 1.0] if c.get("signed") else [0.0, 1.0],
                     norm=norm_of(case, N) if norm else None, norm_frequency=frequency, **kw)
    pipe = [feat]
    if c.get("pipe") == "PW":
        p = np.random.default_rng(c["seed"] * 100 + 1).random((S, N), dtype=np.float32)
        pipe.insert(0, ns.Probability(f"prob_{tag}", torch.from_numpy((np.float32(0.5) + np.float32(0.5) * p).astype(np.float32))))
    ckw = {} if not c.get("average_update") else dict(average_update=c["average_update"], continues_update=False)
    # (built before add_layer sets the layers' batch size: the rule then reduces over the batch with torch.sum at every B)
    return ns.MulticompartmentConnection(src, dst, device="cpu", pipeline=pipe, **ckw)


def build(ns, case, frequency="time step", norm=True):
    """The case's network; `frequency` = "sample" gives its end-of-sample twin, norm=False the same without any norm."""
    c = CASES[case]
    graph = c.get("graph", "ff")
    net = ns.Network(dt=c.get("dt", 1.0), batch_size=c["B"])
    X = ns.Input(n=c["S"], traces=True, tc_trace=20.0)
    Y = _target(ns, c, c["N"])
    layers, conns = [("X", X)], []
    if graph == "two_inputs":
        X2 = ns.Input(n=c["S"] - 9, traces=True, tc_trace=20.0)
        layers.append(("X2", X2))
        conns.append(("X2", "Y", _connection(ns, case, "x2y", X2, Y, frequency, norm)))
    conns.insert(0, ("X", "Y", _connection(ns, case, "xy", X, Y, frequency, norm)))
    layers.append(("Y", Y))
    if graph == "two_layer":
        Z = _target(ns, c, 9)
        layers.append(("Z", Z))
        conns.append(("Y", "Z", _connection(ns, case, "yz", Y, Z, frequency, norm)))
    for name, layer in layers:
        net.add_layer(layer, name=name)
    for src, dst, conn in conns:
        net.add_connection(conn, source=src, target=dst)
    if not c.get("train", True):
        net.train(False)
    return net


def inputs(case, r):
    """Input `r` of a case: {input layer: u8 [T, B, n]} Bernoulli spikes from numpy's generator."""
    c = CASES[case]
    rng = np.random.default_rng(1000 * c["seed"] + r + 7)
    out = {"X": (rng.random((c["T"], c["B"], c["S"])) < c["density"]).astype(np.uint8)}
    if c.get("graph") == "two_inputs":
        out["X2"] = (rng.random((c["T"], c["B"], c["S"] - 9)) < c["density"]).astype(np.uint8)
    return out


def run_kwargs(case, r):
    c = CASES[case]
    return dict(reward=c["rewards"][r], a_plus=A_PLUS, a_minus=A_MINUS) if "rewards" in c else {}


def weights(net):
    """{"<source>_<target>": the connection's Weight feature}."""
    return {f"{s}_{d}": next(f for f in conn.pipeline if type(f).__name__ == "Weight") for (s, d), conn in net.connections.items()}


def _np(t):
    return t.detach().cpu().numpy().copy()


def snapshot(net, rasters):
    out = {f"raster_{l}": np.asarray(r, np.uint8) for l, r in rasters.items()}
    for lname, layer in net.layers.items():
        for k in ("v", "refrac_count", "x", "theta"):
            t = getattr(layer, k, None)
            if isinstance(t, torch.Tensor):
                out[f"{k}_{lname}"] = _np(t).astype(np.float32)
    for (s, d), conn in net.connections.items():
        for k, f in enumerate(conn.pipeline):
            out[f"feat_{s}_{d}_{k}"] = _np(f.value).astype(np.float32)
    for key, feat in weights(net).items():
        rule = feat.learning_rule
        for name in STATE + RINGS:
            t = getattr(rule, name, None)
            if isinstance(t, torch.Tensor):
                out[f"{name}_{key}"] = _np(t).astype(np.float32).reshape(-1)
        for name in INDICES:
            if hasattr(rule, name) and getattr(rule, "average_update", 0):
                out[f"{name}_{key}"] = np.int64(getattr(rule, name))
    out["rng"] = torch.get_rng_state().numpy().copy()
    return out


def run(ns, net, case, device=None, n_in=INPUTS):
    """The case's inputs through net.run with a reset between them; one snapshot per input."""
    c = CASES[case]
    T, B = c["T"], c["B"]
    out = []
    for r in range(n_in):
        mons = {l: ns.Monitor(layer, ["s"], time=T) for l, layer in net.layers.items() if not l.startswith("X")}
        for l, m in mons.items():
            net.add_monitor(m, name=l + "_mon")
        x = {k: torch.from_numpy(v) if device is None else torch.from_numpy(v).to(device) for k, v in inputs(case, r).items()}
        net.run(x, time=run_time(T, c.get("dt", 1.0)), one_step=bool(c.get("one_step", False)), **run_kwargs(case, r))
        out.append(snapshot(net, {l: m.get("s").cpu().numpy().reshape(T, B, -1).astype(np.uint8) for l, m in mons.items()}))
        for l in mons:
            del net.monitors[l + "_mon"]
        net.reset_state_variables()
    return out


def at_bound(case, got):
    """The fraction of the final weights that lie at a bound of their range."""
    lo, hi = (-1.0, 1.0) if CASES[case].get("signed") else (0.0, 1.0)
    ws = [v for k, v in got[-1].items() if k.startswith("feat_") and not (CASES[case].get("pipe") == "PW" and k.endswith("_0"))]
    n = sum(w.size for w in ws)
    return sum(int(((w == lo) | (w == hi)).sum()) for w in ws) / max(n, 1)


def conditions(case, got, sample):
    """What a fixture must show on the reference's own output, so that no case is vacuous.  `sample`: the same case with
    norm_frequency="sample"."""
    c = CASES[case]
    for r, g in enumerate(got):
        for k, v in g.items():
            if k.startswith("raster_"):
                assert v.sum() > 0, f"{case}: {k} has no spikes in input {r + 1}"
    if case == "a":
        assert any(not np.array_equal(g["raster_Y"], s["raster_Y"]) for g, s in zip(got, sample)), "a: the rasters equal the sample mode's"
    if c["rule"] is not None:
        assert any(not np.array_equal(got[-1][k], sample[-1][k]) for k in got[-1] if k.startswith("feat_")), f"{case}: the weights equal the sample mode's"
        frac = at_bound(case, got)
        assert frac < 0.25, f"{case}: {100 * frac:.1f} % of the final weights lie at a bound"


def pack(case, got):
    out = {}
    for r, g in enumerate(got):
        for key, a in g.items():
            out[f"{case}/{key}/{r}"] = np.packbits(a) if key.startswith("raster_") else a
    return out


_GOLD = {}


def gold(case, here):
    """The stored arrays of one case as a list of per-input dicts (rasters unpacked)."""
    import os
    c = CASES[case]
    path = os.path.join(here, "golden", f"norm_step_{case}.npz")
    if path not in _GOLD:
        _GOLD[path] = dict(np.load(path))
    out = []
    for r in range(INPUTS):
        g = {k.split("/")[1]: v for k, v in _GOLD[path].items() if k.startswith(case + "/") and k.endswith(f"/{r}")}
        for k in list(g):
            if k.startswith("raster_"):
                n = g["v_" + k[len("raster_"):]].shape[-1]
                g[k] = np.unpackbits(g[k])[:c["T"] * c["B"] * n].reshape(c["T"], c["B"], n)
        out.append(g)
    return out


def assert_same(case, got, want, what="", skip=()):
    """Bit for bit: rasters, layer state, feature values, rule state, generator state."""
    for r, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), (case, what, sorted(set(g) ^ set(w)))
        for key in w:
            if key in skip:
                continue
            a, b = np.asarray(g[key]), np.asarray(w[key])
            assert a.shape == b.shape and np.array_equal(a, b), f"{case} {what}: {key} differs after input {r + 1}" + \
                (f" ({int((a != b).sum())} of {a.size} elements, max |d| {np.abs(a - b).max():.3g})" if a.dtype == np.float32 and a.shape == b.shape else "")
