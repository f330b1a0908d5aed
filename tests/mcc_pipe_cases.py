"""The feature-pipeline fixture cases (tests/golden/make_golden_mcc_pipe.py), written once for both implementations: `build(ns,
case)` constructs a case's network from a namespace of classes -- the reference's (the generator) or this package's (the tests)
-- and `run_case` drives it with two consecutive inputs (reset_state_variables() in between) and records, per input, every
layer's raster, the final v / refrac_count / traces, every feature value and the global generator's state.

graph "ff"         Input X (S, traces) -> MulticompartmentConnection(pipeline) -> LIFNodes Y (N, traces)
graph "reservoir"  the shape of examples/mnist/MCC_reservoir.py scaled down: X -> Y (per-neuron thresholds) -> Y, both connections
                   [Probability, Weight]
graph "dc"         the DiehlAndCook2015 wiring with [Probability, Weight] on X -> Ae: the Bernoulli draws and the one_spike draws
                   of DiehlAndCookNodes interleave in one generator stream

A pipeline is a string over P (Probability) M (Mask) W (Weight) B (Bias) I (Intensity); the values come from numpy's generator,
so the torch generator is consumed by the run alone.  The `l*` cases cross the kernels' boundaries: S*N below / at / above 624
and no multiple of it (a 624-word block straddles two connections and two timesteps), N = 31 / 32 / 33 / 70 (bit-row padding,
cascade / row_sum column split), S on both sides of 16 and 256 (the flush boundaries of the ordered sum)."""
import hashlib
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time

CASES = {
    "a": dict(graph="reservoir", S=36, N=20, B=1, T=30, pipe="PW", density=0.3, wscale=2.5, seed=31),
    "b": dict(graph="reservoir", S=36, N=20, B=3, T=30, pipe="PW", density=0.3, wscale=2.5, seed=32),
    "c": dict(graph="ff", S=36, N=20, B=2, T=30, pipe="MW", density=0.3, wscale=1.6, seed=33),
    "d": dict(graph="ff", S=36, N=20, B=2, T=30, pipe="PMWB", density=0.3, wscale=3.0, seed=34),
    "e": dict(graph="ff", S=36, N=20, B=1, T=30, pipe="IW", density=0.3, wscale=3.0, seed=35),
    "f": dict(graph="ff", S=36, N=20, B=2, T=30, pipe="WP", density=0.3, wscale=2.5, seed=36),
    "g": dict(graph="ff", S=36, N=20, B=2, T=30, pipe="PPW", density=0.3, wscale=4.0, seed=37),
    "h": dict(graph="ff", S=36, N=20, B=2, T=30, pipe="PW", density=0.3, wscale=2.5, seed=38, rule=True, norm=30.0),
    "i": dict(graph="dc", S=36, N=20, B=2, T=30, pipe="PW", density=0.3, wscale=0.0, seed=39),
    "j": dict(graph="ff", S=36, N=20, B=2, T=30, pipe="P", density=0.3, wscale=0.0, seed=40, pscale=1.0),
    "k": dict(graph="reservoir", S=36, N=20, B=1, T=30, pipe="PW", density=0.3, wscale=2.5, seed=31, one_step=True),
    "l_below": dict(graph="ff", S=17, N=31, B=2, T=20, pipe="PW", density=0.4, wscale=4.0, seed=41),          # 527 < 624
    "l_at": dict(graph="reservoir", S=39, N=16, B=2, T=20, pipe="PW", density=0.3, wscale=2.5, seed=42),        # 39 * 16 = 624; + 256
    "l_above": dict(graph="ff", S=19, N=33, B=2, T=20, pipe="PW", density=0.4, wscale=4.0, seed=43),          # 627 = 624 + 3
    "l_n32": dict(graph="ff", S=15, N=32, B=2, T=20, pipe="PWB", density=0.4, wscale=5.0, seed=44),            # S below 16, one full word per row
    "l_wide": dict(graph="ff", S=300, N=70, B=2, T=12, pipe="PMW", density=0.1, wscale=1.5, seed=45),          # S > 256, N > 64 and no multiple of 32
    "l_bias": dict(graph="ff", S=260, N=37, B=2, T=12, pipe="WB", density=0.1, wscale=1.0, seed=46),           # the dense walk past 256 terms
}
# (h) at dt = 0.5 (default 1.0; `time = T * dt` is run): the refractory countdown, the decays, and MCC PostPre's `* dt` behind a
# Probability feature.  `sibling`: the dt = 1 case it repeats.
CASES["h_dt05"] = dict(CASES["h"], dt=0.5, T=40, B=1, sibling="h")
FEATURES = {"P": "Probability", "M": "Mask", "W": "Weight", "B": "Bias", "I": "Intensity"}
MIN_SPIKES = 36            # "a few dozen": what the generator demands of the reference's own run of every case

# constructor cases: (seed, class letter, S, N) with value=None, primed by a connection Input(S) -> LIFNodes(N)
CTOR = [(51, "P", 7, 9), (52, "M", 30, 40), (53, "B", 7, 9), (54, "I", 7, 9), (55, "W", 7, 9)]


def ns_from(nodes, topology, features, mcc_learning, network_cls, models):
    return SimpleNamespace(Input=nodes.Input, LIFNodes=nodes.LIFNodes, MulticompartmentConnection=topology.MulticompartmentConnection,
                           Probability=features.Probability, Mask=features.Mask, Weight=features.Weight, Bias=features.Bias,
                           Intensity=features.Intensity, PostPre=mcc_learning.PostPre, Network=network_cls,
                           DiehlAndCook2015=models.DiehlAndCook2015)


def make_pipeline(ns, c, S, N, tag, rng):
    """The case's features for one [S, N] connection; `rng` is numpy's generator (values never touch torch's)."""
    out = []
    for k, ch in enumerate(c["pipe"]):
        name = f"{tag}_{k}_{ch}"
        if ch == "P":
            p = (0.2 + 0.8 * rng.random((S, N), dtype=np.float32) * np.float32(c.get("pscale", 0.9))).astype(np.float32)
            out.append(ns.Probability(name, torch.from_numpy(np.minimum(p, np.float32(1.0)))))
        elif ch == "M":
            out.append(ns.Mask(name, torch.from_numpy(rng.random((S, N)) < 0.7)))
        elif ch == "W":
            w = (rng.random((S, N), dtype=np.float32) * np.float32(c["wscale"])).astype(np.float32)
            if tag == "rec":
                w = (w * np.float32(0.2) - np.float32(0.15 * c["wscale"])).astype(np.float32)       # mostly inhibitory recurrence
            kw = dict(range=[0.0, float(c["wscale"])], nu=(1e-3, 1e-2), learning_rule=ns.PostPre, norm=c["norm"]) if c.get("rule") else {}
            out.append(ns.Weight(name, torch.from_numpy(w), **kw))
        elif ch == "B":
            out.append(ns.Bias(name, torch.from_numpy(((rng.random((S, N), dtype=np.float32) - np.float32(0.45)) * np.float32(0.02)).astype(np.float32))))
        else:
            out.append(ns.Intensity(name, torch.from_numpy(rng.integers(-1, 2, (S, N)).astype(np.float32))))
    return out


def build(ns, name):
    c = CASES[name]
    S, N = c["S"], c["N"]
    rng = np.random.default_rng(c["seed"])
    torch.manual_seed(c["seed"])
    if c["graph"] == "dc":
        net = ns.DiehlAndCook2015(n_inpt=S, n_neurons=N, exc=22.5, inh=17.5, dt=1.0, norm=20.0, theta_plus=0.05, nu=(1e-3, 1e-2))
        conn = net.connections[("X", "Ae")]
        conn.pipeline[0].learning_rule.reduction = torch.sum      # (the constructors take the default for batch size 1)
        conn.pipeline[0].value *= 6.0            # weights that make Ae cross its threshold at this input size
        conn.pipeline[0].value.clamp_(0.0, 1.0)
        p = (0.5 + 0.5 * rng.random((S, N), dtype=np.float32)).astype(np.float32)
        feat = ns.Probability("prob", torch.from_numpy(p))
        conn.pipeline.insert(0, feat)
        feat.prime_feature(connection=conn, device="cpu")
        conn.feature_index["prob"] = feat
        return net
    net = ns.Network(dt=c.get("dt", 1.0))
    X = ns.Input(n=S, traces=True, tc_trace=20.0)
    if c["graph"] == "reservoir":
        thresh = (-52.0 + rng.standard_normal(N)).astype(np.float32)
        Y = ns.LIFNodes(n=N, thresh=torch.from_numpy(thresh), traces=True, tc_trace=20.0)
    else:
        Y = ns.LIFNodes(n=N, traces=True, tc_trace=20.0)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    pipe = make_pipeline(ns, c, S, N, "in", rng)
    net.add_connection(ns.MulticompartmentConnection(X, Y, device="cpu", pipeline=pipe), source="X", target="Y")
    if c.get("rule"):
        for f in pipe:
            if isinstance(f, ns.Weight):
                f.learning_rule.reduction = torch.sum             # (the constructor takes the default for batch size 1)
    if c["graph"] == "reservoir":
        net.add_connection(ns.MulticompartmentConnection(Y, Y, device="cpu", pipeline=make_pipeline(ns, c, N, N, "rec", rng)),
                           source="Y", target="Y")
    return net


def inputs(name, r):
    """Input `r` of a case: u8 [T, B, S] Bernoulli spikes from numpy's generator."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c["seed"] + r + 7)
    return (rng.random((c["T"], c["B"], c["S"])) < c["density"]).astype(np.uint8)


def features(net):
    """{"<source>_<target>_<index>": value} of every feature of every connection."""
    out = {}
    for (src, dst), conn in net.connections.items():
        for k, f in enumerate(conn.pipeline):
            out[f"{src}_{dst}_{k}"] = f.value
    return out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def snapshot(net, rasters):
    f = lambda t: t.detach().cpu().numpy().copy()      # noqa: E731
    out = {f"raster_{l}": np.asarray(r, np.uint8) for l, r in rasters.items()}
    for lname, layer in net.layers.items():
        for k in ("v", "refrac_count", "x", "theta"):
            t = getattr(layer, k, None)
            if isinstance(t, torch.Tensor):
                out[f"{k}_{lname}"] = f(t).astype(np.float32)
    for key, val in features(net).items():
        out[f"feat_{key}"] = f(val)
    out["rng"] = torch.get_rng_state().numpy().copy()
    return out


def run_case(net, name, monitor_cls, device=None, n_in=2):
    c = CASES[name]
    T, B = c["T"], c["B"]
    out = []
    for r in range(n_in):
        mons = {l: monitor_cls(layer, ["s"], time=T) for l, layer in net.layers.items() if l != "X"}
        for l, m in mons.items():
            net.add_monitor(m, name=l + "_mon")
        x = torch.from_numpy(inputs(name, r).copy())
        if device is not None:
            x = x.to(device)
        net.run({"X": x}, time=run_time(T, c.get("dt", 1.0)), one_step=bool(c.get("one_step", False)))
        out.append(snapshot(net, {l: m.get("s").cpu().numpy().reshape(T, B, -1).astype(np.uint8) for l, m in mons.items()}))
        for l in mons:
            del net.monitors[l + "_mon"]
        net.reset_state_variables()
    return out


def ctor_case(ns, seed, letter, S, N):
    """A feature with value=None primed by a connection Input(S) -> LIFNodes(N): {"value", "rng"} as numpy, or {"raises": the
    exception's type name, "rng"} where priming fails."""
    torch.manual_seed(seed)
    feat = getattr(ns, FEATURES[letter])("f")
    try:
        ns.MulticompartmentConnection(ns.Input(n=S), ns.LIFNodes(n=N), device="cpu", pipeline=[feat])
    except Exception as e:               # noqa: BLE001
        return {"raises": np.array(type(e).__name__), "rng": torch.get_rng_state().numpy().copy()}
    return {"value": feat.value.detach().numpy().copy(), "rng": torch.get_rng_state().numpy().copy()}


# constructor calls that must raise what the reference raises: name -> callable(ns)
def raising_cases():
    t = torch.full((3, 4), 0.5)
    return {
        "probability_scalar": lambda ns: ns.Probability("f", 0.5),
        "probability_above_one": lambda ns: ns.Probability("f", t + 1.0),
        "probability_negative_min": lambda ns: ns.Probability("f", t, range=[-1, 1]),
        "mask_float_tensor": lambda ns: ns.Mask("f", t),
        "mask_int_scalar": lambda ns: ns.Mask("f", 1),
        "bias_scalar": lambda ns: ns.Bias("f", 0.5),
        "intensity_out_of_range": lambda ns: ns.Intensity("f", t * 4.0),
        "intensity_scalar": lambda ns: ns.Intensity("f", 0.5),
        "probability_wrong_shape": lambda ns: ns.MulticompartmentConnection(ns.Input(n=3), ns.LIFNodes(n=5), device="cpu",
                                                                            pipeline=[ns.Probability("f", t)]),
        "bad_range_order": lambda ns: ns.Bias("f", t, range=[1.0, 0.0]),
    }
