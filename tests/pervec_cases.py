"""The per-neuron parameter fixture cases (tests/golden/make_golden_pervec.py), written once for both implementations:
`build(ns, case)` constructs a case's network from a namespace of classes -- the reference's (the generator) or this package's
(the tests) -- and `run_case` drives it and records, after every input, the Y raster and every state tensor.

Every connection is a MulticompartmentConnection with one Weight (the sum order the other fixtures pin); inputs and the
per-neuron values come from numpy's generator.  A parameter given as a tensor has the layer's shape, one value per neuron.

(a)       LIFNodes n = 70, B = 3, with a recurrent connection: tensor thresh + tc_decay + tc_trace
(b1, b3)  DiehlAndCookNodes shape [5, 9], one_spike: tensor thresh + tc_decay + theta_plus + tc_theta_decay, B = 1 and B = 3
(c)       (b3) under network.train(False)
(d)       AdaptiveLIFNodes n = 300 with additive traces: tensor trace_scale + tc_trace, B = 2
(e_*)     IFNodes, BoostedLIFNodes, CurrentLIFNodes (with tensor tc_i_decay), McCullochPitts, IzhikevichNodes, n = 66, B = 3:
          tensor thresh, plus tc_decay where the class has it
(f)       an Input layer with tensor tc_trace and additive tensor trace_scale, feeding PostPre into LIFNodes: the input trace shows
          up in the weights

MATRIX lists, per class, the parameters tried one at a time as an [n] tensor on the small graph of `matrix_net`: which of them the
reference runs and which it refuses is stored in the fixture `pervec_matrix` and is the contract of both paths."""
import hashlib
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import again, run_time

N_SRC = 40

CASES = {
    "a": dict(kind="lif", shape=[70], B=3, T=60, n_in=2, density=0.25, scale=1.6, seed=31, recurrent=True,
              vec=("thresh", "tc_decay", "tc_trace")),
    "b1": dict(kind="dc", shape=[5, 9], B=1, T=150, n_in=2, density=0.3, scale=2.2, seed=32,
               vec=("thresh", "tc_decay", "theta_plus", "tc_theta_decay")),
    "b3": dict(kind="dc", shape=[5, 9], B=3, T=80, n_in=2, density=0.3, scale=2.2, seed=33,
               vec=("thresh", "tc_decay", "theta_plus", "tc_theta_decay")),
    "c": dict(kind="dc", shape=[5, 9], B=3, T=80, n_in=2, density=0.3, scale=2.2, seed=33, train=False,
              vec=("thresh", "tc_decay", "theta_plus", "tc_theta_decay")),
    "d": dict(kind="alif", shape=[300], B=2, T=50, n_in=2, density=0.25, scale=1.2, seed=34, additive=True,
              vec=("trace_scale", "tc_trace")),
    "e_if": dict(kind="if", shape=[66], B=3, T=50, n_in=2, density=0.25, scale=1.0, seed=35, vec=("thresh",)),
    "e_boosted": dict(kind="boosted", shape=[66], B=3, T=50, n_in=2, density=0.25, scale=1.0, seed=36, vec=("thresh", "tc_decay")),
    "e_clif": dict(kind="clif", shape=[66], B=3, T=50, n_in=2, density=0.25, scale=0.5, seed=37,
                   vec=("thresh", "tc_decay", "tc_i_decay")),
    "e_mcp": dict(kind="mcp", shape=[66], B=3, T=50, n_in=2, density=0.25, scale=0.13, seed=38, vec=("thresh",)),
    "e_izh": dict(kind="izh", shape=[66], B=3, T=60, n_in=2, density=0.25, scale=3.0, seed=39, vec=("thresh",)),
    "f": dict(kind="lif", shape=[30], B=3, T=50, n_in=2, density=0.25, scale=0.5, seed=40, input_vec=True, postpre=True, vec=()),
}

# dt != 1 (default 1.0; `time = T * dt` is run): one case of each node class with per-neuron decays repeated at dt 0.5 -- exp(-dt / tc)
# is then a per-neuron tensor made when the layer joins the network -- and (a) at dt 0.1 with refrac 1.0: ten f32 subtractions of 0.1f
# per refractory period.  `sibling`: the dt = 1 case it repeats.
for _name in ("a", "b3", "d", "e_clif", "e_izh"):
    CASES[_name + "_dt05"] = dict(CASES[_name], dt=0.5, sibling=_name)
CASES["b3_dt05"].update(T=120, B=2)             # (one_spike: at most one neuron fires per step and sample; 80 steps leave 7 neurons with three spikes;
#                                            B = 2 keeps the file under its sibling's size)
CASES["e_clif_dt05"]["scale"] = 0.2      # (at 0.5 every neuron fires as soon as each ten-step refractory period ends)
CASES["a_dt01"] = dict(CASES["a"], dt=0.1, refrac=1.0, B=2, T=100, sibling="a")

# per kind: the scalar constructor arguments, and per parameter the [lo, hi) range its per-neuron values are drawn from
_KW = {
    "lif": dict(thresh=-52.0, rest=-65.0, reset=-65.0, refrac=5, tc_decay=100.0),
    "dc": dict(thresh=-52.0, rest=-65.0, reset=-60.0, refrac=5, tc_decay=100.0, theta_plus=0.5, tc_theta_decay=200.0),
    "alif": dict(thresh=-52.0, rest=-65.0, reset=-60.0, refrac=3, tc_decay=100.0, theta_plus=0.5, tc_theta_decay=200.0),
    "if": dict(thresh=-52.0, reset=-65.0, refrac=5),
    "boosted": dict(thresh=13.0, refrac=5, tc_decay=100.0),
    "clif": dict(thresh=-52.0, rest=-65.0, reset=-65.0, refrac=5, tc_decay=100.0, tc_i_decay=2.0),
    "mcp": dict(thresh=1.0),
    "izh": dict(),
}
_RANGE = {"tc_decay": (40.0, 160.0), "tc_trace": (8.0, 32.0), "trace_scale": (0.5, 1.5), "theta_plus": (0.1, 0.9),
          "tc_theta_decay": (50.0, 400.0), "tc_i_decay": (1.5, 4.0)}
_THRESH = {"lif": (-56.0, -48.0), "dc": (-56.0, -48.0), "alif": (-56.0, -48.0), "if": (-56.0, -48.0), "boosted": (9.0, 17.0),
           "clif": (-56.0, -48.0), "mcp": (0.6, 1.4), "izh": (25.0, 45.0)}
STATE = ("v", "refrac_count", "x", "theta", "i", "u")          # what a layer may have; stored where it does


def ns_from(nodes, topology, features, mcc_learning, network_cls):
    return SimpleNamespace(Input=nodes.Input, LIFNodes=nodes.LIFNodes, DiehlAndCookNodes=nodes.DiehlAndCookNodes,
                           AdaptiveLIFNodes=nodes.AdaptiveLIFNodes, McCullochPitts=nodes.McCullochPitts, IFNodes=nodes.IFNodes,
                           BoostedLIFNodes=nodes.BoostedLIFNodes, CurrentLIFNodes=nodes.CurrentLIFNodes,
                           IzhikevichNodes=nodes.IzhikevichNodes, MulticompartmentConnection=topology.MulticompartmentConnection,
                           Weight=features.Weight, PostPre=mcc_learning.PostPre, Network=network_cls)


def _cls(ns, kind):
    return {"lif": ns.LIFNodes, "dc": ns.DiehlAndCookNodes, "alif": ns.AdaptiveLIFNodes, "if": ns.IFNodes, "boosted": ns.BoostedLIFNodes,
            "clif": ns.CurrentLIFNodes, "mcp": ns.McCullochPitts, "izh": ns.IzhikevichNodes}[kind]


def vectors(name):
    """{parameter: f32 array of the layer's shape} of the case's layer Y, and of its Input layer for (f)."""
    c = CASES[name]
    rng = np.random.default_rng(5000 + c["seed"])
    out = {}
    for p in c["vec"]:
        lo, hi = _THRESH[c["kind"]] if p == "thresh" else _RANGE[p]
        out[p] = (lo + (hi - lo) * rng.random(c["shape"], dtype=np.float32)).astype(np.float32)
    xin = {}
    if c.get("input_vec"):
        for p in ("tc_trace", "trace_scale"):
            lo, hi = _RANGE[p]
            xin[p] = (lo + (hi - lo) * rng.random(N_SRC, dtype=np.float32)).astype(np.float32)
    return out, xin


def _mcc(ns, A, B_, w, **kw):
    feat = ns.Weight("weight", torch.from_numpy(w), **kw)
    return ns.MulticompartmentConnection(A, B_, device="cpu", pipeline=[feat])


def build(ns, name):
    c = CASES[name]
    torch.manual_seed(c["seed"])
    rng = np.random.default_rng(c["seed"])
    yvec, xvec = vectors(name)
    net = ns.Network(dt=c.get("dt", 1.0))
    X = ns.Input(n=N_SRC, traces=True, traces_additive=bool(xvec), **{k: torch.from_numpy(v.copy()) for k, v in xvec.items()},
                 **({} if xvec else dict(tc_trace=20.0)))
    kw = dict(_KW[c["kind"]])
    if "refrac" in c:
        kw["refrac"] = c["refrac"]
    kw.update({k: torch.from_numpy(v.copy()) for k, v in yvec.items()})
    kw.setdefault("tc_trace", 20.0)
    shape = c["shape"]
    size = dict(n=shape[0]) if len(shape) == 1 else dict(shape=shape)
    Y = _cls(ns, c["kind"])(traces=True, traces_additive=bool(c.get("additive")), **size, **kw)
    n = int(np.prod(shape))
    w = rng.random((N_SRC, n), dtype=np.float32) * np.float32(c["scale"])
    if c.get("postpre"):       # (built before add_layer sets a batch size of 1: the rule then reduces over the batch with torch.sum)
        conn = _mcc(ns, X, Y, w, range=[0.0, float(c["scale"])], nu=(1e-4, 1e-3), learning_rule=ns.PostPre)
    else:
        conn = _mcc(ns, X, Y, w)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(conn, source="X", target="Y")
    if c.get("recurrent"):
        wr = (rng.random((n, n), dtype=np.float32) - np.float32(0.7)) * np.float32(0.8)     # mostly inhibitory
        net.add_connection(_mcc(ns, Y, Y, wr), source="Y", target="Y")
    if c.get("train") is False:
        net.train(False)
    return net


def inputs(name, r):
    """Input `r` of a case: u8 [T, B, N_SRC] spikes from numpy's generator (same draws everywhere)."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c["seed"] + r + 11)
    return (rng.random((c["T"], c["B"], N_SRC)) < c["density"]).astype(np.uint8)


def weights(net):
    return net.connections[("X", "Y")].pipeline[0].value


def snapshot(net, name, raster):
    c = CASES[name]
    Y = net.layers["Y"]
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).copy()      # noqa: E731
    out = dict(raster=np.asarray(raster, np.uint8))
    for k in STATE:
        t = getattr(Y, k, None)
        if isinstance(t, torch.Tensor):
            out[k] = f(t)
    if c["kind"] == "dc":
        out["rng"] = torch.get_rng_state().numpy().copy()           # one_spike draws from the global generator
    if c.get("postpre"):
        out["xX"] = f(net.layers["X"].x)
        out["w"] = f(weights(net))
    return out


DERIVED = ("decay", "trace_decay", "theta_decay", "i_decay")     # what compute_decays() makes with torch.exp on the host


def derived(net):
    """{"X_trace_decay": array, "Y_decay": array, ...}: the per-neuron derived buffers of the case's layers."""
    out = {}
    for lname, layer in net.layers.items():
        for k in DERIVED:
            t = getattr(layer, k, None)
            if isinstance(t, torch.Tensor) and t.numel() > 1:
                out[f"{lname}_{k}"] = t.detach().cpu().numpy().astype(np.float32).copy()
    return out


def load_derived(net, g):
    """Give the layers the reference's own derived buffers from fixture `g`, so that run parity does not depend on the last bit of
    the host's exp() (torch picks its vector exp by the CPU it runs on); compute_decays() itself is pinned by the host tests."""
    for key in g.files:
        if key.startswith("derived_"):
            lname, k = key[len("derived_"):].split("_", 1)
            setattr(net.layers[lname], k, torch.from_numpy(np.array(g[key])))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(net, name, monitor_cls, device=None):
    """Run the case's inputs (reset_state_variables() between them); one snapshot per input."""
    c = CASES[name]
    out = []
    torch.manual_seed(100 + c["seed"])                              # where the one_spike draws start
    for r in range(c["n_in"]):
        mon = monitor_cls(net.layers["Y"], ["s"], time=c["T"])
        net.add_monitor(mon, name="Y_mon")
        x = torch.from_numpy(inputs(name, r))
        if device is not None:
            x = x.to(device)
        net.run({"X": x}, time=run_time(c["T"], c.get("dt", 1.0)))
        raster = mon.get("s").cpu().numpy().reshape(c["T"], c["B"], -1).astype(np.uint8)
        out.append(snapshot(net, name, raster))
        del net.monitors["Y_mon"]
        net.reset_state_variables()
    return out


def conditions(name, rasters, thetas=None):
    """What makes a case a test of anything -- asserted by the generator on the reference's output and again by the tests on the
    fixture: per input at least 50 spikes, fewer than half of all (step, neuron) slots spiking, at least two neurons with different
    spike counts; for the (b) cases, thresholds theta that differ between neurons."""
    for r, raster in enumerate(rasters):
        total, counts = int(raster.sum()), raster.reshape(-1, raster.shape[-1]).sum(0)
        assert total >= 50, f"case {name} input {r}: only {total} spikes"
        assert 2 * total < raster.size, f"case {name} input {r}: {total} of {raster.size} slots spike"
        assert len(set(counts.tolist())) >= 2, f"case {name} input {r}: every neuron spikes {counts[0]} times"
    if "dt" in CASES[name] and CASES[name]["kind"] not in ("mcp", "izh"):
        for r, raster in enumerate(rasters):       # a refractory period ended and the neuron fired again, twice
            assert again(raster) >= 10, f"case {name} input {r}: only {again(raster)} neurons spike three or more times"
    if CASES[name].get("sibling", name) in ("b1", "b3") and thetas is not None:
        for r, th in enumerate(thetas):
            assert len(set(np.asarray(th).reshape(-1).tolist())) >= 2, f"case {name} input {r}: theta is the same for every neuron"


# ---- the acceptance matrix -----------------------------------------------------------------------------------------------------
M_SRC, M_N, M_T = 20, 12, 12
MATRIX = {
    "Input": ("tc_trace", "trace_scale", "trace_scale+additive"),
    "McCullochPitts": ("thresh", "tc_trace", "trace_scale", "trace_scale+additive"),
    "IFNodes": ("thresh", "reset", "refrac", "lbound", "tc_trace", "trace_scale", "trace_scale+additive"),
    "LIFNodes": ("thresh", "rest", "reset", "refrac", "tc_decay", "lbound", "tc_trace", "trace_scale", "trace_scale+additive"),
    "BoostedLIFNodes": ("thresh", "refrac", "tc_decay", "tc_trace", "trace_scale", "trace_scale+additive"),
    "CurrentLIFNodes": ("thresh", "rest", "reset", "refrac", "tc_decay", "tc_i_decay", "lbound", "tc_trace", "trace_scale",
                        "trace_scale+additive"),
    "AdaptiveLIFNodes": ("thresh", "rest", "reset", "refrac", "tc_decay", "theta_plus", "tc_theta_decay", "lbound", "tc_trace",
                         "trace_scale", "trace_scale+additive"),
    "DiehlAndCookNodes": ("thresh", "rest", "reset", "refrac", "tc_decay", "theta_plus", "tc_theta_decay", "lbound", "tc_trace",
                          "trace_scale", "trace_scale+additive"),
    "IzhikevichNodes": ("thresh", "rest", "lbound", "tc_trace", "trace_scale", "trace_scale+additive"),
}
_M_BASE = {"thresh": -52.0, "rest": -65.0, "reset": -65.0, "refrac": 5.0, "lbound": -70.0, "tc_decay": 100.0, "tc_i_decay": 2.0,
           "tc_trace": 20.0, "trace_scale": 1.0, "theta_plus": 0.05, "tc_theta_decay": 1e3}
_M_THRESH = {"McCullochPitts": 1.0, "BoostedLIFNodes": 13.0, "IzhikevichNodes": 30.0}
_M_SCALE = {"McCullochPitts": 0.3, "IzhikevichNodes": 6.0}


def matrix_pairs():
    return [f"{cls}:{p}" for cls, params in MATRIX.items() for p in params]


def matrix_net(ns, pair):
    """Input(20) -> MulticompartmentConnection with one Weight -> 12 neurons of the pair's class, its parameter an [n] tensor (on the
    Input layer itself for the Input rows)."""
    cls, param = pair.split(":")
    additive = param.endswith("+additive")
    param = param.split("+")[0]
    n = M_SRC if cls == "Input" else M_N
    base = _M_THRESH.get(cls, _M_BASE[param]) if param == "thresh" else _M_BASE[param]
    value = torch.from_numpy((np.float32(base) + np.float32(0.01 * abs(base)) * np.arange(n, dtype=np.float32)).astype(np.float32))
    torch.manual_seed(7)
    net = ns.Network(dt=1.0)
    if cls == "Input":
        X = ns.Input(n=M_SRC, traces=True, traces_additive=additive, **{param: value})
        Y = ns.LIFNodes(n=M_N, traces=True)
    else:
        X = ns.Input(n=M_SRC, traces=True)
        kw = {} if param == "thresh" or cls not in _M_THRESH else {"thresh": _M_THRESH[cls]}
        Y = getattr(ns, cls)(n=M_N, traces=True, traces_additive=additive, **{param: value}, **kw)
    w = np.random.default_rng(3).random((M_SRC, M_N), dtype=np.float32) * np.float32(_M_SCALE.get(cls, 2.5))
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(_mcc(ns, X, Y, w), source="X", target="Y")
    return net


def matrix_input(B, r):
    return (np.random.default_rng(900 + 10 * B + r).random((M_T, B, M_SRC)) < 0.3).astype(np.uint8)


def matrix_run(ns, pair, device=None):
    """The trial of one pair: B = 1 and B = 3, two runs each with reset_state_variables() between them.  Returns the final v and the
    spike counts of every run; raises what the implementation raises."""
    out = []
    for B in (1, 3):
        net = matrix_net(ns, pair)
        if device is not None:
            net.to(device)
        torch.manual_seed(8)
        for r in range(2):
            x = torch.from_numpy(matrix_input(B, r))
            net.run({"X": x if device is None else x.to(device)}, time=M_T)
            Y, X = net.layers["Y"], net.layers["X"]
            out.append((Y.v.detach().cpu().numpy().copy(), Y.x.detach().cpu().numpy().copy(), X.x.detach().cpu().numpy().copy(),
                        Y.s.detach().cpu().numpy().copy()))
            net.reset_state_variables()
    return out
