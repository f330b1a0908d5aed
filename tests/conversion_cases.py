"""The bindsnet.conversion fixture cases (tests/golden/make_golden_conversion.py), written once for both implementations:
`build(ns, name, ...)` makes a case's network from a namespace of classes -- the reference's (the generator) or this package's (the
tests) --, `run_case` drives it and records every field, and `stated_run` computes the same fields in plain torch / numpy from the
case's own description (`graph`), with no package code: the dense sum over the spiking sources in ascending order with the bias
last (include/snnhip.h, snn_prop_dense_f32), torch's own conv2d and max_pool2d (the orders the existing Conv2dConnection and
MaxPool2dConnection kernels are pinned to), and the step of conversion/nodes.py operation by operation.

Two families.  Dyadic: weights and biases are multiples of 2^-6 in [-1, 1], thresh 1, reset 0 -- every partial sum, v and summed is
exact in f32 in any order, so the device equals the REFERENCE in every field.  Float: ordinary random weights -- the device equals
the stated order bit for bit, and the stated order equals the reference in rasters, refrac_count and traces, with v and summed
within the spreads the generator measured and stored.

Cases (`CASES`): `step_*` one SubtractiveResetIFNodes layer driven by an external current; `g_*` hand-built gather graphs;
`mlp_*`, `cnn_*` networks made by ann_to_snn; `refnet_*` the reference's own test network (784-256-128-10, functional ReLU)."""
import hashlib
import warnings
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from dt_cases import run_time

f32 = np.float32

# ---- step-kernel cases: N, B, refrac, dt, lbound, traces (None / "set" / "add" / "pv": additive with a per-neuron trace_scale), sum_input
STEP = {
    "step_n1": dict(N=1, B=1, refrac=0, dt=1.0, lbound=None, traces=None, sum=True),
    "step_n255": dict(N=255, B=3, refrac=2, dt=1.0, lbound=-0.75, traces="set", sum=False),
    "step_n257": dict(N=257, B=3, refrac=2, dt=0.5, lbound=None, traces="add", sum=True),
    "step_n600": dict(N=600, B=1, refrac=0, dt=0.5, lbound=-0.75, traces="pv", sum=True),
}
STEP_T = 24

# ---- hand-built gather graphs: X Input(src) [-> Connection -> H SIF(src)] -> gather -> P PassThroughNodes -> Connection -> Y SIF(6, sum_input)
GATHER = {
    "g_perm_0312": dict(src=(2, 3, 5), dims=(0, 3, 1, 2)),
    "g_perm_0231": dict(src=(2, 3, 5), dims=(0, 2, 3, 1)),
    "g_perm_0132": dict(src=(2, 3, 5), dims=(0, 1, 3, 2)),
    "g_perm_rank1": dict(src=(7,), dims=(0, 1)),
    "g_pad_1221": dict(src=(2, 3, 5), pad=(1, 2, 2, 1)),
    "g_pad_0000": dict(src=(2, 3, 5), pad=(0, 0, 0, 0)),
    "g_pad_spiking": dict(src=(2, 3, 5), pad=(1, 2, 2, 1), hidden=True),
}
GATHER_T, GATHER_B, GATHER_OUT = 20, 2, 6

# ---- converted networks: arch, family, B, T, one_step, input rate
NETS = {
    "mlp_dy_b1": dict(arch="mlp", family="dyadic", B=1, T=60, rate=0.3),
    "mlp_dy_b3": dict(arch="mlp", family="dyadic", B=3, T=60, rate=0.3),
    "mlp_dy_b3_one": dict(arch="mlp", family="dyadic", B=3, T=60, rate=0.3, one_step=True),
    "mlp_fl_b1": dict(arch="mlp", family="float", B=1, T=60, rate=0.3),
    "mlp_fl_b3": dict(arch="mlp", family="float", B=3, T=60, rate=0.3),
    "mlp_fl_b1_one": dict(arch="mlp", family="float", B=1, T=60, rate=0.3, one_step=True),
    "cnn_dy": dict(arch="cnn", family="dyadic", B=2, T=40, rate=0.3),
    "cnn_fl": dict(arch="cnn", family="float", B=2, T=40, rate=0.3, data=True),       # the weights ann_to_snn(data=...) produced in the reference
    "refnet_plain": dict(arch="refnet", family="float", B=1, T=20, rate=0.5),
    "refnet_data": dict(arch="refnet", family="float", B=1, T=20, rate=0.5, data=True),
}
CASES = list(STEP) + list(GATHER) + list(NETS)
FLOAT = [n for n, c in NETS.items() if c["family"] == "float"]
N_IN = 2                  # inputs per case, reset_state_variables() between them
MARGIN = 8                # every |v - thresh| of a float case is at least MARGIN x v_spread away (CSRM's margin)
INPUT_SHAPE = {"mlp": (50,), "cnn": (1, 12, 12), "refnet": (784,)}


def ns_from(nodes, topology, network_cls, monitor_cls, conversion):
    return SimpleNamespace(Input=nodes.Input, IFNodes=nodes.IFNodes, LIFNodes=nodes.LIFNodes, Connection=topology.Connection,
                           Conv2dConnection=topology.Conv2dConnection, MaxPool2dConnection=topology.MaxPool2dConnection,
                           Network=network_cls, Monitor=monitor_cls, SIF=conversion.SubtractiveResetIFNodes,
                           Pass=conversion.PassThroughNodes, PermuteConnection=conversion.PermuteConnection,
                           PadConnection=conversion.ConstantPad2dConnection, Permute=conversion.Permute,
                           ann_to_snn=conversion.ann_to_snn, data_based_normalization=conversion.data_based_normalization)


def seed_of(name):
    return 700 + CASES.index(name)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dyadic(rng, *shape):
    """Multiples of 2^-6 in [-1, 1]."""
    return (rng.integers(-64, 65, size=shape) / 64.0).astype(f32)


# ---- the cases' own descriptions ----------------------------------------------------------------------------------------------

class RefNet(nn.Module):
    """The network of the reference's test/conversion: 784-256-128-10, ReLU applied in forward(), no Sequential."""

    def __init__(self):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = nn.Linear(784, 256), nn.Linear(256, 128), nn.Linear(128, 10)

    def forward(self, x):
        return self.fc3(F.relu(self.fc2(F.relu(self.fc1(x)))))


def make_ann(name, seed=None):
    """The torch model of a converted case, its parameters set from the case's seed (float family: `seed` from the fixture)."""
    c = NETS[name]
    seed = seed_of(name) if seed is None else int(seed)
    torch.manual_seed(seed)
    if c["arch"] == "refnet":
        ann = RefNet()
        with torch.no_grad():                       # (the default initialisation, scaled so that every layer spikes within T steps)
            for p in ann.parameters():
                p *= 3.0
        return ann
    if c["arch"] == "mlp":
        ann = nn.Sequential(nn.Linear(50, 40), nn.ReLU(), nn.Linear(40, 30), nn.ReLU(), nn.Linear(30, 10))
    else:
        ann = nn.Sequential(nn.ConstantPad2d(1, 0), nn.Conv2d(1, 4, 3), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(4, 6, 3), nn.ReLU(), nn.Linear(96, 10))
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for p in ann.parameters():
            if c["family"] == "dyadic":
                p.copy_(torch.from_numpy(dyadic(rng, *p.shape)))
            else:
                p.copy_(torch.from_numpy(((rng.random(p.shape) * 2 - 1) * (0.5 if p.dim() > 1 else 0.2)).astype(f32)))
    return ann


def stores_params(name):
    """Whether the case's fixture holds the parameters the reference's normalisation produced (float activations: their last
    bits belong to the machine that made them).  The reference's test network is left unscaled by the normalisation -- a
    top-level Linear never becomes the layer to rescale --, so its `data` case normalises for itself."""
    return name in NETS and bool(NETS[name].get("data")) and NETS[name]["arch"] == "cnn"


def norm_data(name):
    """The data a `data=True` case is normalised with."""
    rng = np.random.default_rng(seed_of(name) + 5000)
    return torch.from_numpy(rng.random((16, *INPUT_SHAPE[NETS[name]["arch"]])).astype(f32))


def set_params(ann, arrays):
    with torch.no_grad():
        for p, a in zip(ann.parameters(), arrays):
            p.copy_(torch.from_numpy(np.asarray(a, f32)))
    return ann


def graph_of_ann(ann, input_shape):
    """The plain description of what ann_to_snn makes of `ann` (written from the issue's contract, independently of the package):
    a list of (layer name, kind, source name, parameters), layers named after the child's position."""
    children = []
    for c in ann.children():
        children += list(c.children()) if isinstance(c, nn.Sequential) else [c]
    graph, prev, shape = [], "Input", tuple(input_shape)
    for i, m in enumerate(children, start=1):
        last = i == len(children)
        if isinstance(m, nn.Linear):
            graph.append((str(i), "dense", prev, dict(w=m.weight.detach().numpy().T.copy(), b=m.bias.detach().numpy().copy(), shape=(m.out_features,), sum=last)))
        elif isinstance(m, nn.Conv2d):
            out = (m.out_channels, shape[1] - m.kernel_size[0] + 1, shape[2] - m.kernel_size[1] + 1)
            graph.append((str(i), "conv", prev, dict(w=m.weight.detach().numpy().copy(), b=m.bias.detach().numpy().copy(), shape=out, sum=last)))
        elif isinstance(m, nn.MaxPool2d):
            graph.append((str(i), "pool", prev, dict(k=m.kernel_size, shape=(shape[0], shape[1] // m.kernel_size, shape[2] // m.kernel_size))))
        elif isinstance(m, nn.ConstantPad2d):
            p = m.padding
            graph.append((str(i), "pad", prev, dict(pad=tuple(p), shape=(shape[0], shape[1] + p[2] + p[3], shape[2] + p[0] + p[1]))))
        else:
            continue
        prev, shape = str(i), graph[-1][3]["shape"]
    return graph


def gather_weights(name):
    c = GATHER[name]
    rng = np.random.default_rng(seed_of(name))
    n = int(np.prod(c["src"]))
    out = gather_out_shape(name)
    wy, by = dyadic(rng, int(np.prod(out)), GATHER_OUT), dyadic(rng, GATHER_OUT)
    wh = bh = None
    if c.get("hidden"):
        wh, bh = dyadic(rng, n, n), dyadic(rng, n)
    return wh, bh, wy, by


def gather_out_shape(name):
    c = GATHER[name]
    if "dims" in c:
        return tuple(c["src"][d - 1] for d in c["dims"][1:])
    l, r, t, b = c["pad"]
    return (c["src"][0], c["src"][1] + t + b, c["src"][2] + l + r)


def graph_of_gather(name):
    c = GATHER[name]
    wh, bh, wy, by = gather_weights(name)
    graph, prev = [], "X"
    if c.get("hidden"):
        graph.append(("H", "dense", "X", dict(w=wh, b=bh, shape=tuple(c["src"]), sum=False)))
        prev = "H"
    if "dims" in c:
        graph.append(("P", "permute", prev, dict(dims=c["dims"], shape=gather_out_shape(name))))
    else:
        graph.append(("P", "pad", prev, dict(pad=c["pad"], shape=gather_out_shape(name))))
    graph.append(("Y", "dense", "P", dict(w=wy, b=by, shape=(GATHER_OUT,), sum=True)))
    return graph


def step_layer_kwargs(name):
    c = STEP[name]
    kw = dict(n=c["N"], thresh=1.0, reset=0.0, refrac=c["refrac"], lbound=c["lbound"], sum_input=c["sum"])
    if c["traces"]:
        kw.update(traces=True, traces_additive=c["traces"] in ("add", "pv"), tc_trace=8.0)
        kw["trace_scale"] = torch.linspace(0.5, 1.5, c["N"]) if c["traces"] == "pv" else 0.75
    return kw


def step_currents(name, r):
    """[T, B, N] f32 currents, multiples of 2^-4: step 0 drives every neuron exactly to the threshold (all spike), step 1 is
    negative (none spikes), later steps are mixed and at times push v below `lbound`."""
    c = STEP[name]
    rng = np.random.default_rng(1000 * seed_of(name) + r)
    cur = (rng.integers(-24, 25, size=(STEP_T, c["B"], c["N"])) / 16.0).astype(f32)
    cur[0], cur[1] = 1.0, -0.5
    cur[5] = -1.25                                  # (below lbound = -0.75 for every neuron that is not refractory)
    return cur


def spikes(name, r, shape, T, B, rate):
    rng = np.random.default_rng(1000 * seed_of(name) + r)
    return (rng.random((T, B, *shape)) < rate).astype(np.uint8)


def case_meta(name):
    """(input layer name or None, input shape, T, B, dt, one_step)."""
    if name in STEP:
        c = STEP[name]
        return None, (c["N"],), STEP_T, c["B"], c["dt"], False
    if name in GATHER:
        return "X", tuple(GATHER[name]["src"]), GATHER_T, GATHER_B, 1.0, False
    c = NETS[name]
    return "Input", INPUT_SHAPE[c["arch"]], c["T"], c["B"], 1.0, bool(c.get("one_step"))


def case_inputs(name, r):
    inp, shape, T, B, dt, _ = case_meta(name)
    if inp is None:
        return {"Y": torch.from_numpy(step_currents(name, r))}
    rate = NETS[name]["rate"] if name in NETS else 0.4
    return {inp: torch.from_numpy(spikes(name, r, shape, T, B, rate))}


# ---- building and running with a class namespace --------------------------------------------------------------------------------

def set_batch(net, B):
    """A network made at another batch size (ann_to_snn: 1) taken to B before its first run, pooling rates included -- run() itself
    resizes the layers only, and the pooling connections of both implementations then refuse their stale rates."""
    if net.batch_size != B:
        net.batch_size = B
        for l in net.layers.values():
            l.set_batch_size(B)
        for c in net.connections.values():
            c.reset_state_variables()


def build(ns, name, params=None, seed=None, eval_mode=False):
    """The case's network.  `params`: the fixture's arrays for a case whose weights the reference's normalisation produced.
    eval_mode: network.train(False) -- the generator's call: in training mode the reference's NoOp multiplies the `w` a pooling,
    permuting or padding connection does not have (AttributeError); this package runs them in training mode, so the tests do not."""
    net = _build(ns, name, params, seed)
    if eval_mode:
        net.train(False)
    return net


def _build(ns, name, params, seed):
    inp, shape, T, B, dt, _ = case_meta(name)
    if name in STEP:
        net = ns.Network(dt=dt, batch_size=B)
        net.add_layer(ns.SIF(**step_layer_kwargs(name)), name="Y")
        return net
    if name in GATHER:
        c = GATHER[name]
        wh, bh, wy, by = gather_weights(name)
        net = ns.Network(dt=1.0, batch_size=B)
        net.add_layer(ns.Input(shape=c["src"]), name="X")
        prev = "X"
        if c.get("hidden"):
            net.add_layer(ns.SIF(shape=c["src"], thresh=1.0, reset=0.0, refrac=0), name="H")
            net.add_connection(ns.Connection(net.layers["X"], net.layers["H"], w=torch.from_numpy(wh), b=torch.from_numpy(bh)), "X", "H")
            prev = "H"
        net.add_layer(ns.Pass(shape=list(gather_out_shape(name))), name="P")
        if "dims" in c:
            conn = ns.PermuteConnection(net.layers[prev], net.layers["P"], dims=c["dims"])
        else:
            conn = ns.PadConnection(net.layers[prev], net.layers["P"], padding=c["pad"])
        net.add_connection(conn, prev, "P")
        net.add_layer(ns.SIF(n=GATHER_OUT, thresh=1.0, reset=0.0, refrac=0, sum_input=True), name="Y")
        net.add_connection(ns.Connection(net.layers["P"], net.layers["Y"], w=torch.from_numpy(wy), b=torch.from_numpy(by)), "P", "Y")
        return net
    ann = make_ann(name, seed)
    if params is not None:
        set_params(ann, params)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        net = ns.ann_to_snn(ann, shape, data=norm_data(name) if NETS[name].get("data") and params is None else None)      # (params: already normalised)
    set_batch(net, B)
    return net


def graph(name, params=None, seed=None):
    if name in STEP:
        return [("Y", "current", None, dict(shape=(STEP[name]["N"],), sum=STEP[name]["sum"]))]
    if name in GATHER:
        return graph_of_gather(name)
    ann = make_ann(name, seed)
    if params is not None:
        set_params(ann, params)
    return graph_of_ann(ann, INPUT_SHAPE[NETS[name]["arch"]])


def net_params(net):
    """w and b of every weighted connection, in order: what a fixture stores of a network the reference normalised."""
    out = []
    for conn in net.connections.values():
        if hasattr(conn, "w"):
            w = conn.w.detach().cpu().numpy()
            out += [w.T.copy() if w.ndim == 2 else w.copy(), conn.b.detach().cpu().numpy().copy()]      # (back in the ANN's layout)
    return out


def _np(t):
    return t.detach().cpu().numpy().astype(f32).copy()


def snapshot(net, rasters, vrecs):
    out = {}
    for lname, layer in net.layers.items():
        if lname in rasters:
            out[f"{lname}_raster"] = rasters[lname]
        if lname in vrecs:
            out[f"{lname}_vrec"] = vrecs[lname]
        if hasattr(layer, "refrac_count"):
            out[f"{lname}_v"], out[f"{lname}_rc"] = _np(layer.v), _np(layer.refrac_count)
        if getattr(layer, "traces", False) and hasattr(layer, "refrac_count"):
            out[f"{lname}_x"] = _np(layer.x)
        if getattr(layer, "sum_input", False):
            out[f"{lname}_summed"] = _np(layer.summed)
    for (src, dst), conn in net.connections.items():
        if hasattr(conn, "firing_rates"):
            out[f"{dst}_fr"] = _np(conn.firing_rates)
    return out


def run_case(ns, net, name, device=None, first=0, count=None, halves=False, record_v=True):
    """Run inputs [first, first + count) with reset_state_variables() between them; one snapshot per input.  halves: every input as
    two runs under one monitor.  The rasters of all non-Input layers and (record_v) the per-step v of the spiking ones are recorded."""
    inp, shape, T, B, dt, one_step = case_meta(name)
    count = N_IN - first if count is None else count
    out = []
    for r in range(first, first + count):
        mons = {}
        for lname, layer in net.layers.items():
            if lname == inp:
                continue
            mons[lname, "s"] = ns.Monitor(layer, ["s"], time=T)
            if record_v and hasattr(layer, "refrac_count"):
                mons[lname, "v"] = ns.Monitor(layer, ["v"], time=T)
        for key, m in mons.items():
            net.add_monitor(m, name="_".join(key))
        x = {k: (v.to(device) if device is not None else v) for k, v in case_inputs(name, r).items()}
        if halves:
            h = T // 2
            net.run({k: v[:h].clone() for k, v in x.items()}, time=run_time(h, dt), one_step=one_step)
            net.run({k: v[h:].clone() for k, v in x.items()}, time=run_time(T - h, dt), one_step=one_step)
        else:
            net.run(x, time=run_time(T, dt), one_step=one_step)
        rasters = {l: (m.get("s").cpu().numpy().reshape(T, B, -1) != 0).astype(np.uint8) for (l, v), m in mons.items() if v == "s"}
        vrecs = {l: m.get("v").cpu().numpy().reshape(T, B, -1).astype(f32) for (l, v), m in mons.items() if v == "v"}
        out.append(snapshot(net, rasters, vrecs))
        for key in mons:
            del net.monitors["_".join(key)]
        net.reset_state_variables()
    return out


# ---- the stated order, in plain torch / numpy ------------------------------------------------------------------------------------

def dense_stated(s, w, b):
    """out[b, j] = (((0 + w[i1, j]) + w[i2, j]) + ...) + b[j] over the spiking sources i1 < i2 < ..., one rounded f32 add per term."""
    B = s.shape[0]
    out = np.zeros((B, w.shape[1]), f32)
    for k in range(B):
        acc = np.zeros(w.shape[1], f32)
        for i in np.flatnonzero(s[k].reshape(-1)):
            acc = acc + w[i]
        out[k] = acc + b
    return out


def sif_stated(st, x, thresh, refrac, dt, lbound):
    """One step of conversion/nodes.py:81-97 on numpy f32 arrays; returns (spikes, v before the reset)."""
    dt = f32(dt)
    st["v"] = st["v"] + (st["rc"] == 0).astype(f32) * x
    st["rc"] = (st["rc"] > 0).astype(f32) * (st["rc"] - dt)
    pre = st["v"].copy()
    s = st["v"] >= f32(thresh)
    st["rc"][s] = f32(refrac)
    st["v"][s] = st["v"][s] - f32(thresh)
    if lbound is not None:
        st["v"][st["v"] < f32(lbound)] = f32(lbound)
    return s.astype(np.uint8), pre


def stated_run(name, params=None, seed=None, first=0, count=None):
    """The case in the stated order: the snapshots run_case returns (rasters, per-step v, final v / rc / x / summed, firing_rates),
    plus per spiking layer `<L>_margin`, the least |v - thresh| met before a reset."""
    g = graph(name, params, seed)
    inp, shape, T, B, dt, one_step = case_meta(name)
    count = N_IN - first if count is None else count
    kw = step_layer_kwargs(name) if name in STEP else dict(thresh=1.0, refrac=0, lbound=None)
    trace = None
    if name in STEP and STEP[name]["traces"]:
        decay = torch.exp(-torch.tensor(dt) / torch.tensor(kw["tc_trace"])).numpy().astype(f32)      # (compute_decays' own expression)
        scale = kw["trace_scale"].numpy().astype(f32) if isinstance(kw["trace_scale"], torch.Tensor) else f32(kw["trace_scale"])
        trace = (decay, scale, kw["traces_additive"])
    out = []
    for r in range(first, first + count):
        x_in = case_inputs(name, r)
        state, spk = {}, {}
        for lname, kind, src, p in g:
            n = int(np.prod(p["shape"]))
            spk[lname] = np.zeros((B, n), np.uint8)
            if kind in ("dense", "conv", "current"):
                state[lname] = dict(v=np.zeros((B, n), f32), rc=np.zeros((B, n), f32), summed=np.zeros((B, n), f32), x=np.zeros((B, n), f32),
                                    margin=np.inf)
        if inp is not None:
            spk[inp] = np.zeros((B, int(np.prod(shape))), np.uint8)
        rec = {lname: np.zeros((T, B, spk[lname].shape[1]), np.uint8) for lname, *_ in g}
        vrec = {lname: np.zeros((T, B, spk[lname].shape[1]), f32) for lname in state}
        fr = {}
        src_shape = {inp: shape} if inp is not None else {}
        for lname, kind, src, p in g:
            src_shape[lname] = p["shape"]

        def current(lname, kind, src, p):
            s = spk[src] if src is not None else None
            if kind == "current":
                return x_in["Y"][t].numpy().reshape(B, -1).astype(f32)
            if kind == "dense":
                return dense_stated(s, p["w"], p["b"])
            s4 = torch.from_numpy(s.reshape(B, *src_shape[src]))
            if kind == "conv":
                return F.conv2d(s4.float(), torch.from_numpy(p["w"]), torch.from_numpy(p["b"])).numpy().reshape(B, -1)
            if kind == "pool":                     # decay = 1: the rates ARE the last spikes, the gathered spike is the window's maximum
                fr[lname] = s4.float().numpy().copy()
                return F.max_pool2d(s4.float(), p["k"]).numpy().reshape(B, -1)
            if kind == "permute":
                return s4.permute(p["dims"]).float().numpy().reshape(B, -1)
            return F.pad(s4, p["pad"]).float().numpy().reshape(B, -1)

        for t in range(T):
            cur = {}
            if not one_step:
                for lname, kind, src, p in g:
                    cur[lname] = current(lname, kind, src, p)
            if inp is not None:
                spk[inp] = x_in[inp][t].numpy().reshape(B, -1)
            for lname, kind, src, p in g:
                if one_step:
                    cur[lname] = current(lname, kind, src, p)
                if lname in state:
                    st = state[lname]
                    s, pre = sif_stated(st, cur[lname], kw["thresh"], kw["refrac"], dt, kw["lbound"])
                    st["margin"] = min(st["margin"], float(np.abs(pre.astype(np.float64) - kw["thresh"]).min()))
                    if trace is not None:
                        st["x"] = st["x"] * trace[0]
                        if trace[2]:
                            st["x"] = st["x"] + trace[1] * s.astype(f32)
                        else:
                            st["x"][s != 0] = trace[1]
                    if p.get("sum"):
                        st["summed"] = st["summed"] + cur[lname]
                    vrec[lname][t] = st["v"]
                else:
                    s = (cur[lname] != 0).astype(np.uint8)
                spk[lname] = s
                rec[lname][t] = s
        snap = {}
        for lname, kind, src, p in g:
            snap[f"{lname}_raster"] = rec[lname]
            if lname in state:
                st = state[lname]
                snap[f"{lname}_vrec"], snap[f"{lname}_v"], snap[f"{lname}_rc"] = vrec[lname], st["v"].reshape(B, *p["shape"]), st["rc"].reshape(B, *p["shape"])
                snap[f"{lname}_margin"] = st["margin"]
                if trace is not None:
                    snap[f"{lname}_x"] = st["x"].reshape(B, *p["shape"])
                if p.get("sum"):
                    snap[f"{lname}_summed"] = st["summed"].reshape(B, *p["shape"])
            if lname in fr:
                snap[f"{lname}_fr"] = fr[lname]
        out.append(snap)
    return out


def spiking_layers(name):
    return [l for l, kind, _, _ in graph(name) if kind in ("dense", "conv", "current")]


# ---- integer-valued normalisation cases: every activation is exact in f32, so the scaled parameters are the reference's on any CPU ---

def norm_case(kind):
    """(model with small integer weights, integer-valued data, input shape)."""
    rng = np.random.default_rng(31 if kind == "mlp" else 32)
    if kind == "mlp":
        ann = nn.Sequential(nn.Sequential(nn.Linear(12, 8), nn.ReLU(), nn.Linear(8, 6), nn.ReLU()), nn.Linear(6, 4))
        shape = (12,)
    else:
        ann = nn.Sequential(nn.Conv2d(1, 3, 3), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(3, 4, 3), nn.ReLU(), nn.Linear(36, 5))
        shape = (1, 12, 12)
    with torch.no_grad():
        for p in ann.parameters():
            p.copy_(torch.from_numpy(rng.integers(-3, 4, size=tuple(p.shape)).astype(f32)))
    data = torch.from_numpy(rng.integers(0, 4, size=(10, *shape)).astype(f32))
    return ann, data, shape


# ---- calls whose outcome the generator records ("ok" or the exception's name) --------------------------------------------------------

def _quiet(fn):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return fn()


def _run_net(net, shape, B=1, T=3):
    set_batch(net, B)
    x = (np.random.default_rng(5).random((T, B, *shape)) < 0.5).astype(np.uint8)
    net.run({"Input": torch.from_numpy(x)}, time=T)
    return net


CALLS = {
    # a Permute child: the helper indexes prev.shape with the batch-inclusive dims
    "permute_child_0231": lambda ns: _quiet(lambda: ns.ann_to_snn(nn.Sequential(ns.Permute((0, 2, 3, 1)), nn.Linear(30, 4)), (2, 3, 5))),
    "permute_child_021": lambda ns: _run_net(_quiet(lambda: ns.ann_to_snn(nn.Sequential(ns.Permute((0, 2, 1)), nn.Linear(30, 4)), (2, 3, 5))), (2, 3, 5)),
    # a Conv2d without bias: zeros(layer.shape[1]), one per output row
    "conv_no_bias": lambda ns: _run_net(_quiet(lambda: ns.ann_to_snn(nn.Sequential(nn.Conv2d(1, 4, 3, bias=False), nn.ReLU(), nn.Linear(144, 3)), (1, 8, 8))), (1, 8, 8)),
    "conv_no_bias_square": lambda ns: _run_net(_quiet(lambda: ns.ann_to_snn(nn.Sequential(nn.Conv2d(1, 6, 3, bias=False), nn.ReLU(), nn.Linear(216, 3)), (1, 8, 8))), (1, 8, 8)),
    # the pad shape adds padding[0] + padding[1] to the height
    "pad_asymmetric": lambda ns: _run_net(_quiet(lambda: ns.ann_to_snn(nn.Sequential(nn.ConstantPad2d((1, 2, 0, 0), 0), nn.Linear(66, 3)), (2, 3, 8))), (2, 3, 8)),
    "pad_symmetric": lambda ns: _run_net(_quiet(lambda: ns.ann_to_snn(nn.Sequential(nn.ConstantPad2d(1, 0), nn.Linear(100, 3)), (2, 3, 8))), (2, 3, 8)),
    "node_type_if": lambda ns: _quiet(lambda: ns.ann_to_snn(nn.Sequential(nn.Linear(5, 4), nn.ReLU(), nn.Linear(4, 3)), (5,), node_type=ns.IFNodes)),
    "sum_input_on_input": lambda ns: ns.Input(n=3, sum_input=True),
    "no_data_warns": lambda ns: _warns(ns),
    "one_child": lambda ns: _quiet(lambda: ns.ann_to_snn(nn.Sequential(nn.Linear(5, 4)), (5,))),
    "no_children": lambda ns: _quiet(lambda: ns.ann_to_snn(nn.Sequential(), (5,))),
}


def _warns(ns):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ns.ann_to_snn(nn.Sequential(nn.Linear(5, 4), nn.ReLU(), nn.Linear(4, 3)), (5,))
    assert any(issubclass(x.category, RuntimeWarning) for x in w), "no RuntimeWarning without data"


def outcome(ns, call):
    try:
        CALLS[call](ns)
    except Exception as e:         # noqa: BLE001  (the point is to record which)
        return type(e).__name__
    return "ok"
