"""The real-valued (analog) Input fixture cases (tests/golden/make_golden_analog.py), written once for both implementations:
`build(ns, name, ...)` makes a case's network from a namespace of classes -- the reference's (the generator) or this package's (the
tests) --, `run_case` drives it with float32 inputs and records every field, and `stated_run` computes the same fields in numpy from
the case's own description, with no package code.  The stated order of include/snnhip.h (f17) is restated here: `dense_real_stated`
(source index ascending, one rounded multiply and one rounded add per term, bias last) and `conv2d_real_stated` (one sequential sum
over (kh, kw, cin), input channel innermost, bias last).

Two families, as tests/conversion_cases.py.  Dyadic: inputs are multiples of 1/16 in [0, 1], weights and biases multiples of 1/64 in
[-1, 1], thresh 1, reset 0 -- every product, partial sum, v and summed is exact in f32 (`assert_dyadic`), so the device equals the
REFERENCE in every field.  Float: ordinary weights and inputs -- the device equals the stated order bit for bit, the stated order
equals the reference in rasters, refrac_count and traces, and v / summed lie within the spreads the generator measured and stored.

Cases (`CASES`): `mlp_*`, `cnn_*` networks made by ann_to_snn; `tr_*` a hand-built Input -> Connection -> LIFNodes graph with traces
on the Input; `left_*` two runs without a reset in between, one fed bytes and one fed floats."""
import math
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from conversion_cases import dense_stated, dyadic, ns_from, set_batch, sha, sif_stated     # noqa: F401  (re-exported for the tests)

f32 = np.float32

# ---- converted networks: arch, family, B, T, one_step; repeat: the same sample at every step (encoding.repeat), else a new one per step
NETS = {
    "mlp_dy_b1": dict(arch="mlp", family="dyadic", B=1, T=60, repeat=True),
    "mlp_dy_b3_one": dict(arch="mlp", family="dyadic", B=3, T=60, one_step=True),
    "mlp_fl_b1": dict(arch="mlp", family="float", B=1, T=60, repeat=True),
    "mlp_fl_b3": dict(arch="mlp", family="float", B=3, T=60),
    "cnn_dy": dict(arch="cnn", family="dyadic", B=2, T=40),
    "cnn_fl": dict(arch="cnn", family="float", B=2, T=40),
}
# ---- Input(30, traces) -> Connection -> LIFNodes(16, traces): the Input's trace mode ("pv": additive with a per-neuron trace_scale)
TRACE = {"tr_set": dict(mode="set"), "tr_add": dict(mode="add"), "tr_pv": dict(mode="pv")}
TRACE_IN, TRACE_OUT, TRACE_B, TRACE_T = 30, 16, 3, 30
LIF = dict(thresh=-64.0, rest=-65.0, reset=-65.0, refrac=2, tc_decay=100.0, tc_trace=20.0)
# ---- Input(20) -> Connection -> SIF(12, sum_input): two runs, NO reset in between; what the first / the second run is fed
LEFT = {"left_byte_float": ("byte", "float"), "left_float_byte": ("float", "byte")}
LEFT_IN, LEFT_OUT, LEFT_B, LEFT_T = 20, 12, 2, 10

CASES = list(NETS) + list(TRACE) + list(LEFT)
FLOAT = [n for n, c in NETS.items() if c["family"] == "float"]
N_IN = 2                  # inputs per case, reset_state_variables() between them
MARGIN = 8                # every |v - thresh| of a float case is at least MARGIN x v_spread away
INPUT_SHAPE = {"mlp": (50,), "cnn": (1, 12, 12)}


def seed_of(name):
    return 900 + CASES.index(name)


# ---- the cases' own descriptions ----------------------------------------------------------------------------------------------

def make_ann(name, seed=None):
    c = NETS[name]
    seed = seed_of(name) if seed is None else int(seed)
    torch.manual_seed(seed)
    if c["arch"] == "mlp":
        ann = nn.Sequential(nn.Linear(50, 40), nn.ReLU(), nn.Linear(40, 30), nn.ReLU(), nn.Linear(30, 10))
    else:
        ann = nn.Sequential(nn.Conv2d(1, 4, 3), nn.ReLU(), nn.MaxPool2d(2), nn.Linear(100, 10))
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for p in ann.parameters():
            if c["family"] == "dyadic":
                p.copy_(torch.from_numpy(dyadic(rng, *p.shape)))
            else:
                p.copy_(torch.from_numpy(((rng.random(p.shape) * 2 - 1) * (0.5 if p.dim() > 1 else 0.2)).astype(f32)))
    return ann


def hand_weights(name):
    """(w [Nin, N], b [N]) of a hand-built case: dyadic."""
    rng = np.random.default_rng(seed_of(name))
    nin, n = (TRACE_IN, TRACE_OUT) if name in TRACE else (LEFT_IN, LEFT_OUT)
    return dyadic(rng, nin, n), dyadic(rng, n)


def trace_scale(name):
    mode = TRACE[name]["mode"]
    return torch.linspace(0.5, 1.5, TRACE_IN) if mode == "pv" else 0.75


def case_meta(name):
    """(input layer name, input shape, T, B, one_step)."""
    if name in TRACE:
        return "X", (TRACE_IN,), TRACE_T, TRACE_B, False
    if name in LEFT:
        return "X", (LEFT_IN,), LEFT_T, LEFT_B, False
    c = NETS[name]
    return "Input", INPUT_SHAPE[c["arch"]], c["T"], c["B"], bool(c.get("one_step"))


def is_dyadic(name):
    return name not in FLOAT


def analog_values(name, r, part=0):
    """[T, B, *shape] float32: about 40 % exact zeros (image-like), the rest multiples of 1/16 in (0, 1] (dyadic family) or
    uniform in (0, 1) (float family)."""
    inp, shape, T, B, _ = case_meta(name)
    rng = np.random.default_rng(1000 * seed_of(name) + 10 * r + part)
    steps = 1 if name in NETS and NETS[name].get("repeat") else T
    if is_dyadic(name):
        x = (rng.integers(1, 17, size=(steps, B, *shape)) / 16.0).astype(f32)
    else:
        x = (0.02 + 0.98 * rng.random((steps, B, *shape))).astype(f32)
    x = x * (rng.random(x.shape) < 0.6)
    return np.ascontiguousarray(np.broadcast_to(x, (T, B, *shape)).astype(f32))


def byte_values(name, r, part=0):
    inp, shape, T, B, _ = case_meta(name)
    rng = np.random.default_rng(1000 * seed_of(name) + 10 * r + part + 5)
    return (rng.random((T, B, *shape)) < 0.4).astype(np.uint8)


def case_runs(name, r):
    """The runs of input r: a list of [T, B, *shape] arrays, float32 or uint8, run one after the other WITHOUT a reset."""
    if name in LEFT:
        return [analog_values(name, r, k) if kind == "float" else byte_values(name, r, k) for k, kind in enumerate(LEFT[name])]
    return [analog_values(name, r)]


# ---- building and running with a class namespace --------------------------------------------------------------------------------

def build(ns, name, seed=None, eval_mode=False):
    """The case's network.  eval_mode: network.train(False) -- the generator's call (the reference's NoOp multiplies the `w` a
    pooling connection does not have in training mode); this package runs them in training mode, so the tests do not."""
    inp, shape, T, B, _ = case_meta(name)
    if name in NETS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            net = ns.ann_to_snn(make_ann(name, seed), shape)
        set_batch(net, B)
    else:
        w, b = hand_weights(name)
        net = ns.Network(dt=1.0, batch_size=B)
        if name in TRACE:
            mode = TRACE[name]["mode"]
            net.add_layer(ns.Input(n=TRACE_IN, traces=True, traces_additive=mode != "set", tc_trace=LIF["tc_trace"], trace_scale=trace_scale(name)), name="X")
            net.add_layer(ns.LIFNodes(n=TRACE_OUT, traces=True, thresh=LIF["thresh"], rest=LIF["rest"], reset=LIF["reset"], refrac=LIF["refrac"],
                                      tc_decay=LIF["tc_decay"], tc_trace=LIF["tc_trace"]), name="Y")
        else:
            net.add_layer(ns.Input(n=LEFT_IN), name="X")
            net.add_layer(ns.SIF(n=LEFT_OUT, thresh=1.0, reset=0.0, refrac=0, sum_input=True), name="Y")
        net.add_connection(ns.Connection(net.layers["X"], net.layers["Y"], w=torch.from_numpy(w), b=torch.from_numpy(b)), "X", "Y")
    if eval_mode:
        net.train(False)
    return net


def _np(t):
    return t.detach().cpu().numpy().astype(f32).copy()


def run_case(ns, net, name, device=None, first=0, count=None, check=None):
    """Run inputs [first, first + count), reset_state_variables() between them; one snapshot per input: the rasters of every
    non-Input layer, the per-step v of the spiking ones, final v / refrac_count / x / summed, the pooling firing_rates, and for the
    `tr_*` cases the Input's per-step trace (`X_xrec`) and final trace (`X_x`).  check(net): called behind every run()."""
    inp, shape, T, B, one_step = case_meta(name)
    count = N_IN - first if count is None else count
    out = []
    for r in range(first, first + count):
        runs = case_runs(name, r)
        total = T * len(runs)
        mons = {}
        for lname, layer in net.layers.items():
            if lname == inp:
                continue
            mons[lname, "s"] = ns.Monitor(layer, ["s"], time=total)
            if hasattr(layer, "refrac_count"):
                mons[lname, "v"] = ns.Monitor(layer, ["v"], time=total)
        if name in TRACE:
            mons[inp, "x"] = ns.Monitor(net.layers[inp], ["x"], time=total)
        for key, m in mons.items():
            net.add_monitor(m, name="_".join(key))
        for x in runs:
            x = torch.from_numpy(x.copy())
            net.run({inp: x.to(device) if device is not None else x}, time=T, one_step=one_step)
            if check is not None:
                check(net)
        snap = {}
        for (l, v), m in mons.items():
            rec = m.get(v).cpu().numpy().reshape(total, B, -1)
            if v == "s":
                snap[f"{l}_raster"] = (rec != 0).astype(np.uint8)
            else:
                snap[f"{l}_{v}rec"] = rec.astype(f32)
        for lname, layer in net.layers.items():
            if hasattr(layer, "refrac_count"):
                snap[f"{lname}_v"], snap[f"{lname}_rc"] = _np(layer.v), _np(layer.refrac_count)
            if getattr(layer, "traces", False):
                snap[f"{lname}_x"] = _np(layer.x)
            if getattr(layer, "sum_input", False):
                snap[f"{lname}_summed"] = _np(layer.summed)
        for (src, dst), conn in net.connections.items():
            if hasattr(conn, "firing_rates"):
                snap[f"{dst}_fr"] = _np(conn.firing_rates)
        out.append(snap)
        for key in mons:
            del net.monitors["_".join(key)]
        net.reset_state_variables()
    return out


# ---- the stated order, in numpy ------------------------------------------------------------------------------------------------

def dense_real_stated(x, w, b=None, prev=None):
    """out[b, j] = (...((0 + x[b,0] * w[0,j]) + x[b,1] * w[1,j]) + ...) (+ b[j]); then `prev + out` (accumulate) or `0 + out`.  Every
    multiply and every add is one rounded f32 operation."""
    x, w = np.asarray(x, f32).reshape(len(x), -1), np.asarray(w, f32)
    acc = np.zeros((x.shape[0], w.shape[1]), f32)
    for i in range(w.shape[0]):
        acc = acc + x[:, i:i + 1] * w[i][None, :]
    if b is not None:
        acc = acc + np.asarray(b, f32)[None, :]
    return (np.zeros_like(acc) if prev is None else np.asarray(prev, f32)) + acc


def conv2d_real_stated(x, w, b=None, stride=1, pad=0, prev=None):
    """One bias-free sequential f32 sum over (kh, kw, cin), input channel innermost, per output element; out-of-image taps are
    zero terms (a +-0 added to a chain that starts at +0 changes nothing for finite weights); bias last; then prev / 0 + that."""
    x, w = np.asarray(x, f32), np.asarray(w, f32)
    B, Cin, H, Wd = x.shape
    Cout, _, KH, KW = w.shape
    OH, OW = (H + 2 * pad - KH) // stride + 1, (Wd + 2 * pad - KW) // stride + 1
    xp = np.zeros((B, Cin, H + 2 * pad, Wd + 2 * pad), f32)
    xp[:, :, pad:pad + H, pad:pad + Wd] = x
    acc = np.zeros((B, Cout, OH, OW), f32)
    for ky in range(KH):
        for kx in range(KW):
            for ci in range(Cin):
                patch = xp[:, ci, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride]
                acc = acc + patch[:, None] * w[None, :, ci, ky, kx, None, None]
    if b is not None:
        acc = acc + np.asarray(b, f32)[None, :, None, None]
    return (np.zeros_like(acc) if prev is None else np.asarray(prev, f32)) + acc


def input_trace_stated(x, s, decay, scale, additive):
    """The Input's trace with real-valued `s`: x * decay, then trace_scale where s != 0, or + trace_scale * s (product rounded first)."""
    x = np.asarray(x, f32) * f32(decay)
    s = np.asarray(s, f32)
    if additive:
        return (x + (np.asarray(scale, f32) * s).astype(f32)).astype(f32)
    x = x.copy()
    x[s != 0] = f32(scale)
    return x


def lif_stated(st, cur, p, dt=1.0):
    """One step of LIFNodes.forward (nodes.py:500-529) on numpy f32 arrays; returns (spikes, v before the reset)."""
    decay = torch.exp(-torch.tensor(dt) / torch.tensor(p["tc_decay"])).numpy().astype(f32)
    st["v"] = decay * (st["v"] - f32(p["rest"])) + f32(p["rest"])
    cur = np.where(st["rc"] > 0, f32(0), cur).astype(f32)
    st["rc"] = st["rc"] - f32(dt)
    st["v"] = st["v"] + cur
    pre = st["v"].copy()
    s = st["v"] >= f32(p["thresh"])
    st["rc"][s] = f32(p["refrac"])
    st["v"][s] = f32(p["reset"])
    return s.astype(np.uint8), pre


def graph(name, seed=None):
    """[(layer, kind, source, parameters)] in network order: "dense" / "conv" into a spiking layer, "pool" into a pass-through."""
    if name not in NETS:
        w, b = hand_weights(name)
        return [("Y", "dense", "X", dict(w=w, b=b, shape=(w.shape[1],), sum=name in LEFT, node="lif" if name in TRACE else "sif"))]
    ann = make_ann(name, seed)
    g, prev, shape = [], "Input", INPUT_SHAPE[NETS[name]["arch"]]
    children = list(ann.children())
    for i, m in enumerate(children, start=1):
        last = i == len(children)
        if isinstance(m, nn.Linear):
            g.append((str(i), "dense", prev, dict(w=m.weight.detach().numpy().T.copy(), b=m.bias.detach().numpy().copy(), shape=(m.out_features,), sum=last, node="sif")))
        elif isinstance(m, nn.Conv2d):
            out = (m.out_channels, shape[1] - m.kernel_size[0] + 1, shape[2] - m.kernel_size[1] + 1)
            g.append((str(i), "conv", prev, dict(w=m.weight.detach().numpy().copy(), b=m.bias.detach().numpy().copy(), shape=out, sum=last, node="sif")))
        elif isinstance(m, nn.MaxPool2d):
            g.append((str(i), "pool", prev, dict(k=m.kernel_size, shape=(shape[0], shape[1] // m.kernel_size, shape[2] // m.kernel_size))))
        else:
            continue
        prev, shape = str(i), g[-1][3]["shape"]
    return g


def stated_run(name, seed=None, first=0, count=None):
    """The case in the stated order: the snapshots run_case returns, plus per spiking layer `<L>_margin`, the least |v - thresh| met
    before a reset."""
    g = graph(name, seed)
    inp, shape, T, B, one_step = case_meta(name)
    count = N_IN - first if count is None else count
    tr = None
    if name in TRACE:
        decay = torch.exp(-torch.tensor(1.0) / torch.tensor(LIF["tc_trace"])).numpy().astype(f32)
        scale = trace_scale(name)
        tr = (decay, scale.numpy().astype(f32) if isinstance(scale, torch.Tensor) else f32(scale), TRACE[name]["mode"] != "set")
    shapes = {inp: shape, **{l: p["shape"] for l, _, _, p in g}}
    out = []
    for r in range(first, first + count):
        runs = case_runs(name, r)
        total = T * len(runs)
        val = {inp: np.zeros((B, int(np.prod(shape))), np.uint8)}          # what connections read of each layer: bytes, or f32 for an analog Input
        state, rec, vrec, fr = {}, {}, {}, {}
        for l, kind, src, p in g:
            n = int(np.prod(p["shape"]))
            val[l] = np.zeros((B, n), np.uint8)
            rec[l] = np.zeros((total, B, n), np.uint8)
            if kind != "pool":
                rest = f32(LIF["rest"]) if p["node"] == "lif" else f32(0)
                state[l] = dict(v=np.full((B, n), rest, f32), rc=np.zeros((B, n), f32), summed=np.zeros((B, n), f32), x=np.zeros((B, n), f32), margin=np.inf)
                vrec[l] = np.zeros((total, B, n), f32)
        x_in = np.zeros((B, int(np.prod(shape))), f32)
        xrec = np.zeros((total, B, int(np.prod(shape))), f32)

        def current(l, kind, src, p):
            s = val[src]
            real = s.dtype == f32
            if kind == "dense":
                return dense_real_stated(s, p["w"], p["b"]) if real else dense_stated(s, p["w"], p["b"])
            s4 = s.reshape(B, *shapes[src])
            if kind == "conv":
                if real:
                    return conv2d_real_stated(s4, p["w"], p["b"]).reshape(B, -1)
                return F.conv2d(torch.from_numpy(s4).float(), torch.from_numpy(p["w"]), torch.from_numpy(p["b"])).numpy().reshape(B, -1)
            fr[l] = s4.astype(f32).copy()              # pool, decay = 1: the rates ARE the last spikes
            return F.max_pool2d(torch.from_numpy(s4).float(), p["k"]).numpy().reshape(B, -1)

        t = 0
        for x in runs:
            for step in range(T):
                cur = {}
                if not one_step:
                    for l, kind, src, p in g:
                        cur[l] = current(l, kind, src, p)
                val[inp] = x[step].reshape(B, -1)
                if tr is not None:
                    x_in = input_trace_stated(x_in, val[inp], *tr)
                    xrec[t] = x_in
                for l, kind, src, p in g:
                    if one_step:
                        cur[l] = current(l, kind, src, p)
                    if l in state:
                        st = state[l]
                        if p["node"] == "lif":
                            s, pre = lif_stated(st, cur[l], LIF)
                            thresh = LIF["thresh"]
                            st["x"] = st["x"] * torch.exp(-torch.tensor(1.0) / torch.tensor(LIF["tc_trace"])).numpy().astype(f32)
                            st["x"][s != 0] = f32(1.0)
                        else:
                            s, pre = sif_stated(st, cur[l], 1.0, 0, 1.0, None)
                            thresh = 1.0
                        st["margin"] = min(st["margin"], float(np.abs(pre.astype(np.float64) - thresh).min()))
                        if p.get("sum"):
                            st["summed"] = st["summed"] + cur[l]
                        vrec[l][t] = st["v"]
                    else:
                        s = (cur[l] != 0).astype(np.uint8)
                    val[l] = s
                    rec[l][t] = s
                t += 1
        snap = {}
        for l, kind, src, p in g:
            snap[f"{l}_raster"] = rec[l]
            if l in state:
                st = state[l]
                snap[f"{l}_vrec"], snap[f"{l}_v"], snap[f"{l}_rc"] = vrec[l], st["v"].reshape(B, *p["shape"]), st["rc"].reshape(B, *p["shape"])
                snap[f"{l}_margin"] = st["margin"]
                if p["node"] == "lif":
                    snap[f"{l}_x"] = st["x"].reshape(B, *p["shape"])
                if p.get("sum"):
                    snap[f"{l}_summed"] = st["summed"].reshape(B, *p["shape"])
            if l in fr:
                snap[f"{l}_fr"] = fr[l]
        if tr is not None:
            snap[f"{inp}_xrec"], snap[f"{inp}_x"] = xrec, x_in.reshape(B, *shape)
        out.append(snap)
    return out


def assert_dyadic(name):
    """The dyadic condition: inputs on the 1/16 grid in [0, 1], weights and biases on the 1/64 grid in [-1, 1], and fan-in and run
    length small enough that every product, partial sum, v and summed has at most 22 significant bits -- exact in f32, in any order."""
    inp, shape, T, B, _ = case_meta(name)
    for r in range(N_IN):
        for x in case_runs(name, r):
            if x.dtype == f32:
                assert np.array_equal(x * 16, np.round(x * 16)) and x.min() >= 0 and x.max() <= 1, name
    steps = T * (len(LEFT[name]) if name in LEFT else 1)
    for l, kind, src, p in graph(name):
        if kind == "pool":
            continue
        for a in (p["w"], p["b"]):
            assert np.array_equal(a * 64, np.round(a * 64)) and np.abs(a).max() <= 1, (name, l)
        fan_in = p["w"].shape[0] if kind == "dense" else int(np.prod(p["w"].shape[1:]))
        assert fan_in <= 50 or (src != inp and fan_in <= 100) or (kind == "conv" and fan_in <= 75), (name, l, fan_in)
        frac = 10 if src == inp else 6             # x * w on the 2^-10 grid out of the analog Input, w on the 2^-6 grid behind spikes
        bits = math.ceil(math.log2(steps * (fan_in + 1))) + frac
        assert bits <= 22, (name, l, bits)
        if p["node"] == "lif":                     # a leaky v is not on a grid: what must be exact is the current (one step's sum)
            assert math.ceil(math.log2(fan_in + 1)) + frac <= 22


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32).reshape(-1)


def gold(name):
    import cases
    return cases.gold("analog_" + name)


def check_snapshots(name, snaps, g, first=0, exact=None):
    """The snapshots of run_case / stated_run against the fixture.  exact: v and summed bit for bit (default: the dyadic family);
    otherwise within the fixture's v_spread / summed_spread.  Rasters, refrac_count and traces always bit for bit."""
    import cases
    exact = name not in FLOAT if exact is None else exact
    seen = 0
    for i, s in enumerate(snaps):
        r = first + i
        for k, v in s.items():
            if k.endswith("_vrec") or k.endswith("_margin"):
                continue
            ref = g[f"r{r}_{k}"]
            seen += 1
            if k.endswith("_raster"):
                want = cases.unpack(ref, v.shape)
                assert 0 < int(want.sum()) < want.size, "a raster that is all zeros or all ones checks nothing"
                assert np.array_equal(np.asarray(v, np.uint8), want), f"case {name} input {r}: {k} differs ({int(np.asarray(v).sum())} vs {int(want.sum())} spikes)"
            elif not exact and (k.endswith("_v") or k.endswith("_summed")):
                spread = float(g["summed_spread" if k.endswith("_summed") else "v_spread"])
                err = float(np.abs(np.asarray(v, np.float64).reshape(-1) - ref.astype(np.float64).reshape(-1)).max())
                assert err <= spread, f"case {name} input {r}: {k} is {err:.3g} from the reference, the measured spread is {spread:.3g}"
            else:
                got, want = _bits(v), _bits(ref)
                assert got.size == want.size and np.array_equal(got, want), f"case {name} input {r}: {k} differs at {np.flatnonzero(got != want)[:5]}"
    assert seen > 0


def same_snapshots(a, b, what):
    """Two lists of snapshots, every field bit for bit."""
    assert len(a) == len(b)
    for r, (p, q) in enumerate(zip(a, b)):
        keys = [k for k in p if not k.endswith("_margin")]
        assert keys and set(keys) <= set(q), (what, sorted(set(keys) - set(q)))
        for k in keys:
            x, y = np.asarray(p[k]), np.asarray(q[k], np.asarray(p[k]).dtype).reshape(np.asarray(p[k]).shape)
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), f"{what}: input {r} {k} differs"


# ---- the operator sweep: shapes and inputs of the dense product and the convolution (host check and device) ---------------------------

DENSE_NIN, DENSE_N, DENSE_B = (1, 255, 257, 1025), (1, 63, 65, 257), (1, 3, 9)
CONV_CIN, CONV_IMG, CONV_K, CONV_STRIDE, CONV_PAD, CONV_COUT, CONV_B = (1, 3, 17), ((5, 7), (12, 12)), (1, 3, 5), (1, 2), (0, 1, 2), (1, 8, 9), (1, 3)
STEP_N, STEP_B, STEP_T = (1, 255, 257), (1, 3), 6


def real_values(rng, B, *shape):
    """[B, *shape] float32 with negative values, values above 1, about half exact zeros, every fifth source zero in all samples
    and, where B > 1, sample 1 zero throughout."""
    x = (rng.standard_normal((B, *shape)) * 1.5).astype(f32)
    x = x * (rng.random(x.shape) < 0.5)
    x.reshape(B, -1)[:, ::5] = 0
    if B > 1:
        x[1] = 0
    return np.ascontiguousarray(x.astype(f32))


def dense_sweep(nin):
    """Every (N, B, bias, accumulate) at this Nin: dicts of x, w, b (or None), prev (or None) and the stated result `want`."""
    out = []
    for n in DENSE_N:
        for B in DENSE_B:
            for bias in (False, True):
                for acc in (False, True):
                    rng = np.random.default_rng(hash((nin, n, B, bias, acc)) % (2 ** 32))
                    c = dict(x=real_values(rng, B, nin), w=rng.standard_normal((nin, n)).astype(f32),
                             b=rng.standard_normal(n).astype(f32) if bias else None, prev=rng.standard_normal((B, n)).astype(f32) if acc else None)
                    c["want"] = dense_real_stated(c["x"], c["w"], c["b"], c["prev"])
                    out.append(c)
    return out


def conv_sweep(cin, img):
    """Every (K, stride, pad, Cout, B) at this Cin and image size; bias and accumulate alternate from case to case."""
    out, k = [], 0
    for K in CONV_K:
        for stride in CONV_STRIDE:
            for pad in CONV_PAD:
                for cout in CONV_COUT:
                    for B in CONV_B:
                        rng = np.random.default_rng(hash((cin, img, K, stride, pad, cout, B)) % (2 ** 32))
                        oh, ow = (img[0] + 2 * pad - K) // stride + 1, (img[1] + 2 * pad - K) // stride + 1
                        c = dict(x=real_values(rng, B, cin, *img), w=rng.standard_normal((cout, cin, K, K)).astype(f32), stride=stride, pad=pad,
                                 b=rng.standard_normal(cout).astype(f32) if k % 2 == 0 else None,
                                 prev=rng.standard_normal((B, cout, oh, ow)).astype(f32) if k % 3 == 0 else None)
                        c["want"] = conv2d_real_stated(c["x"], c["w"], c["b"], stride, pad, c["prev"])
                        out.append(c)
                        k += 1
    return out


def step_sweep():
    """Every (N, B, trace mode) of the Input step: s [T, B, N], decay, scale (scalar or [N]), additive, and the stated traces [T, B, N]."""
    out = []
    for n in STEP_N:
        for B in STEP_B:
            for mode in ("set", "add", "pv"):
                rng = np.random.default_rng(1000 * n + 10 * B + ("set", "add", "pv").index(mode))
                s = np.stack([real_values(rng, B, n) for _ in range(STEP_T)])
                decay = np.exp(f32(-1.0) / f32(8.0)).astype(f32)
                scale = np.linspace(0.5, 1.5, n).astype(f32) if mode == "pv" else f32(0.75)
                x, rec = (rng.standard_normal((B, n)) * 0.25).astype(f32), []
                x0 = x.copy()
                for t in range(STEP_T):
                    x = input_trace_stated(x, s[t], decay, scale, mode != "set")
                    rec.append(x)
                out.append(dict(s=s, x0=x0, decay=float(decay), scale=scale, additive=mode != "set", mode=mode, want=np.stack(rec)))
    return out


def zero_one(a):
    """A float32 array's 0.0 / 1.0 values as bytes (the 0/1 invariance)."""
    a = np.asarray(a)
    assert np.isin(a, (0.0, 1.0)).all()
    return a.astype(np.uint8)
