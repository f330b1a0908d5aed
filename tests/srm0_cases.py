"""The SRM0Nodes / Rmax fixture cases (tests/golden/make_golden_srm0.py), written once for both implementations: `build(ns, case)`
constructs a case's network from a namespace of classes -- the reference's (the generator) or this package's (the tests) -- and
`run_case` drives it and records, per input and per SRM0 layer, the raster, the per-step v (and, stepping one timestep per run(),
the per-step s_prob), every final state tensor, the weights and the rule's eligibility trace, and the global generator's state
before and after.

direct   one SRM0 layer Y driven by run(inputs={"Y": current}).  The shape cases d_b<B>n<n>_w<warm> put B*n below, at and above the
         generator's 624-word block (303; 624; 626; 1285 = two block boundaries per step, n no whole wave), each from a generator
         warmed by 0, 5 and 623 draws (block position "twist first", 5, 623).  lbound / refrac0 / pervec (per-neuron thresh and
         tc_decay) / dt05 / dt2 are the parameter variants.
two      two SRM0 layers A, B in one network: the stream is consumed in layer order within a step.
mcc      Input -> MulticompartmentConnection [Probability, Weight] -> SRM0: the Probability mask is drawn while the inputs are
         gathered, before any layer steps.
conn     Input(40, additive traces) -> Connection -> SRM0(24), B = 1, T = 60: `grid` without a rule and weights on a 1/4 grid (every
         current exact in any summation order), rmax / rmax_neg / rmax_decay with Rmax (reward 1.0 / -0.5; weight_decay and finite
         bounds), rmax_local the same rule on a LocalConnection.
"""
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time

SHAPES = [(1, 24), (3, 101), (1, 624), (2, 313), (5, 257)]
WARMS = (0, 5, 623)

CASES = {}
for _k, (_B, _n) in enumerate(SHAPES):
    for _w in WARMS:
        CASES[f"d_b{_B}n{_n}_w{_w}"] = dict(graph="direct", B=_B, n=_n, T=30, n_in=1, warm=_w, seed=100 + 10 * _k + WARMS.index(_w))
CASES["lbound"] = dict(graph="direct", B=2, n=40, T=30, n_in=2, warm=7, seed=201, lbound=-70.5, cur=(-2.0, 3.5), additive=True)
CASES["refrac0"] = dict(graph="direct", B=2, n=40, T=30, n_in=2, warm=0, seed=202, refrac=0, cur=(-0.5, 1.5))
CASES["pervec"] = dict(graph="direct", B=3, n=37, T=30, n_in=2, warm=11, seed=203, pervec=True)
CASES["dt05"] = dict(graph="direct", B=2, n=40, T=40, n_in=2, warm=3, seed=204, dt=0.5, cur=(-0.25, 1.5))
CASES["dt2"] = dict(graph="direct", B=2, n=40, T=30, n_in=2, warm=3, seed=205, dt=2.0, cur=(-1.0, 5.0))
CASES["two"] = dict(graph="two", B=2, n=40, n2=33, T=30, n_in=2, warm=2, seed=206)
CASES["mcc"] = dict(graph="mcc", B=2, S=30, n=24, T=30, n_in=2, warm=1, seed=207, density=0.3)
CASES["grid"] = dict(graph="conn", B=1, S=40, n=24, T=60, n_in=2, warm=4, seed=301, density=0.25)
CASES["rmax"] = dict(graph="conn", B=1, S=40, n=24, T=60, n_in=2, warm=4, seed=322, density=0.25, rule=True, reward=1.0)
CASES["rmax_neg"] = dict(graph="conn", B=1, S=40, n=24, T=60, n_in=2, warm=9, seed=323, density=0.25, rule=True, reward=-0.5)
CASES["rmax_decay"] = dict(graph="conn", B=1, S=40, n=24, T=60, n_in=2, warm=0, seed=314, density=0.25, rule=True, reward=1.0,
                           weight_decay=0.01, wmin=-0.25, wmax=0.75)
CASES["rmax_local"] = dict(graph="local", B=1, S=40, n=24, T=60, n_in=2, warm=6, seed=325, density=0.25, rule=True, reward=1.0)

NU = 1e-3
RULE_CASES = sorted(k for k, c in CASES.items() if c.get("rule"))
MARGIN = {False: 2.0 ** -20, True: 2.0 ** -14}          # the least |u - s_prob| a fixture may contain: direct and grid cases / Rmax cases


def srm0_layers(name):
    return ("A", "B") if CASES[name]["graph"] == "two" else ("Y",)


def ns_from(nodes, topology, features, learning, network_cls):
    return SimpleNamespace(Input=nodes.Input, SRM0Nodes=nodes.SRM0Nodes, Connection=topology.Connection,
                           LocalConnection=topology.LocalConnection, MulticompartmentConnection=topology.MulticompartmentConnection,
                           Probability=features.Probability, Weight=features.Weight, Rmax=learning.Rmax, Network=network_cls)


def build(ns, name, decay=None):
    """decay: the per-neuron `decay` buffer of the pervec case as the fixture recorded it.  compute_decays() makes it with the host's
    torch.exp, a 1-ulp function whose last bit differs between CPU kinds; the run's parity must not depend on that, so the tests load
    the recorded buffer (the scalar decays are stored too and compared)."""
    net = _build(ns, name)
    if decay is not None:
        for L in srm0_layers(name):
            net.layers[L].decay = torch.from_numpy(np.array(decay[L]))
    return net


def _build(ns, name):
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"])                    # (LocalConnection draws its initial weights from numpy's global generator)
    net = ns.Network(dt=c.get("dt", 1.0))
    kw = dict(traces=True, traces_additive=bool(c.get("additive")), tc_trace=20.0, refrac=c.get("refrac", 5))
    if "lbound" in c:
        kw["lbound"] = c["lbound"]
    if c.get("pervec"):
        kw["thresh"] = torch.from_numpy((-50.0 + 2.0 * rng.standard_normal(c["n"])).astype(np.float32))
        kw["tc_decay"] = torch.from_numpy((8.0 + 6.0 * rng.random(c["n"])).astype(np.float32))
    if c["graph"] == "direct":
        net.add_layer(ns.SRM0Nodes(n=c["n"], **kw), name="Y")
        return net
    if c["graph"] == "two":
        net.add_layer(ns.SRM0Nodes(n=c["n"], **kw), name="A")
        net.add_layer(ns.SRM0Nodes(n=c["n2"], rho_0=0.5, d_thresh=4.0, eps_0=1.5, **kw), name="B")
        return net
    S, n = c["S"], c["n"]
    X = ns.Input(n=S, shape=(1, 5, 8) if c["graph"] == "local" else None, traces=True, traces_additive=True, tc_trace=20.0)
    Y = ns.SRM0Nodes(n=n, **kw)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    if c["graph"] == "mcc":
        p = (0.3 + 0.7 * rng.random((S, n), dtype=np.float32)).astype(np.float32)
        w = (rng.random((S, n), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
        pipe = [ns.Probability("prob", torch.from_numpy(p)), ns.Weight("weight", torch.from_numpy(w))]
        net.add_connection(ns.MulticompartmentConnection(X, Y, device="cpu", pipeline=pipe), source="X", target="Y")
        return net
    rule = dict(update_rule=ns.Rmax, nu=NU, weight_decay=c.get("weight_decay", 0.0)) if c.get("rule") else {}
    if "wmin" in c:
        rule.update(wmin=c["wmin"], wmax=c["wmax"])
    if c["graph"] == "local":       # 5 x 8 input, 3 x 4 receptive fields at stride (2, 4): 2 x 2 positions x 6 filters = 24 targets
        conn = ns.LocalConnection(X, Y, kernel_size=(3, 4), stride=(2, 4), n_filters=6, input_shape=(5, 8), **rule)
    elif c.get("rule"):
        w = (rng.random((S, n), dtype=np.float32) * np.float32(0.3)).astype(np.float32)
        conn = ns.Connection(X, Y, w=torch.from_numpy(w), **rule)
    else:
        w = (rng.integers(0, 3, (S, n)) * 0.25).astype(np.float32)        # 0, 1/4, 1/2: sums of at most 40 of them are exact in f32
        conn = ns.Connection(X, Y, w=torch.from_numpy(w))
    net.add_connection(conn, source="X", target="Y")
    return net


def inputs(name, r):
    """Input `r` of a case, from numpy's generator: f32 [T, B, n] currents per SRM0 layer, or {"X": u8 [T, B, S] spikes}."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c["seed"] + r + 5)
    T, B = c["T"], c["B"]
    if c["graph"] in ("direct", "two"):
        lo, hi = c.get("cur", (-0.5, 3.0))
        out = {}
        for lname, n in zip(srm0_layers(name), (c["n"], c.get("n2"))):
            out[lname] = (lo + (hi - lo) * rng.random((T, B, n), dtype=np.float32)).astype(np.float32)
        return out
    shape = (T, B, 1, 5, 8) if c["graph"] == "local" else (T, B, c["S"])
    return {"X": (rng.random(shape) < c["density"]).astype(np.uint8)}


def weights(net):
    conn = net.connections.get(("X", "Y"))
    if conn is None:
        return None
    return conn.pipeline[1].value if hasattr(conn, "pipeline") else conn.w


def run_kwargs(name):
    c = CASES[name]
    return {"reward": c["reward"]} if c.get("rule") else {}


def _np(t):
    return t.detach().cpu().numpy().astype(np.float32).copy()


def run_case(net, name, monitor_cls, device=None, mode="whole", first=0, count=None):
    """Run inputs [first, first+count) of the case (reset_state_variables() between them); one snapshot per input.  The generator is
    warmed by the case's `warm` draws before input 0.  mode: "whole" -- one run() of T steps; "halves" -- two of T/2;
    "steps" -- T runs of one step each, which also records every layer's s_prob after each step (`<L>_prec`)."""
    c = CASES[name]
    T, dt = c["T"], c.get("dt", 1.0)
    count = c["n_in"] - first if count is None else count
    layers = srm0_layers(name)
    kw = run_kwargs(name)
    if first == 0 and c["warm"]:
        torch.rand(c["warm"])
    out = []
    for r in range(first, first + count):
        mons = {}
        for L in layers:
            mons[L] = monitor_cls(net.layers[L], ["s", "v"], time=T)
            net.add_monitor(mons[L], name=L + "_mon")
        inp = {k: torch.from_numpy(v.copy()) for k, v in inputs(name, r).items()}
        if device is not None:
            inp = {k: v.to(device) for k, v in inp.items()}
        snap = {"rng0": torch.get_rng_state().numpy().copy()}
        cuts = {"whole": [0, T], "halves": [0, T // 2, T], "steps": list(range(T + 1))}[mode]
        prec = {L: [] for L in layers}
        for a, b in zip(cuts[:-1], cuts[1:]):
            net.run({k: v[a:b] for k, v in inp.items()}, time=run_time(b - a, dt), **kw)
            if mode == "steps":
                for L in layers:
                    prec[L].append(_np(net.layers[L].s_prob).reshape(c["B"], -1))
        snap["rng1"] = torch.get_rng_state().numpy().copy()
        for L in layers:
            Y = net.layers[L]
            snap[L + "_raster"] = mons[L].get("s").cpu().numpy().reshape(T, c["B"], -1).astype(np.uint8)
            snap[L + "_vrec"] = mons[L].get("v").cpu().numpy().reshape(T, c["B"], -1).astype(np.float32)
            if mode == "steps":
                snap[L + "_prec"] = np.stack(prec[L])
            snap[L + "_v"], snap[L + "_rc"], snap[L + "_x"] = _np(Y.v), _np(Y.refrac_count), _np(Y.x)
            snap[L + "_sprob"] = _np(Y.s_prob)
            del net.monitors[L + "_mon"]
        if "X" in net.layers:
            snap["xX"] = _np(net.layers["X"].x)
            snap["w"] = _np(weights(net))
        if c.get("rule"):
            snap["e"] = _np(net.connections[("X", "Y")].update_rule.eligibility_trace)
        out.append(snap)
        net.reset_state_variables()
    return out
