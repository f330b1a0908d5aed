"""The time-averaged update fixture cases (tests/golden/make_golden_mcc_average.py), written once for both implementations: the
builders take a namespace of classes -- the reference's (the generator) or this package's (the tests).

Every case is Input S -> MulticompartmentConnection [Weight, range [0, 1], norm, an MCC rule with average_update = K] -> LIF N, run
over INPUTS inputs of T steps with reset_state_variables() between them (the rings are NOT cleared by it: MCC_learning.py:304, :550,
:735-738).  Names: "<rule>_b<B>_k<K>_<w|c>[_<variant>]", w = windowed (continues_update=False), c = continuous.

    main shape   37 x 29: E = 1073 is no multiple of 32, so the ring's mean and the batch reduction cover both ATen column classes
    e1 / e6      1 x 1 and 2 x 3: ATen's inner reduction (E = 1) and the 4 <= E <= 7 class (low LIF thresholds, so that they spike)
    post         PostPre with nu = (0, nu1): only the post ring and its index move
    rvec         MSTDP with one reward per sample

T = 40 is a multiple of none of K = 3, 7, 33: the second input starts in the middle of a ring.  Recorded after every input: the Y
raster, W, the rings, the ring indices, p_plus, p_minus, eligibility_trace."""
from types import SimpleNamespace

import numpy as np
import torch

S, N, T, INPUTS = 37, 29, 40, 2
SHAPES = {"main": (37, 29), "e1": (1, 1), "e6": (2, 3)}
RULES = ("PostPre", "MSTDP", "MSTDPET")
BATCHES, KS = (1, 3, 33), (1, 2, 3, 7, 33)
A_PLUS, A_MINUS = 1.0, -0.6           # (with a_plus == -a_minus the first point eligibility cancels to 0)
REWARDS = (0.8, -0.6)                 # one per input
_NU = {"PostPre": (0.02, 0.05), "MSTDP": (0.06, 0.0), "MSTDPET": (0.8, 0.0)}
RINGS = {"PostPre": (("average_buffer_pre", "average_buffer_index_pre"), ("average_buffer_post", "average_buffer_index_post")),
         "MSTDP": (("average_buffer", "average_buffer_index"),), "MSTDPET": (("average_buffer", "average_buffer_index"),)}
STATE = ("p_plus", "p_minus", "eligibility_trace")


def _cases():
    out = {}
    for ri, rule in enumerate(RULES):
        for B in BATCHES:
            if rule == "MSTDPET" and B != 1:
                continue
            for K in KS:
                for cont in (False, True):
                    out[f"{rule}_b{B}_k{K}_{'c' if cont else 'w'}"] = dict(rule=rule, B=B, K=K, cont=cont, shape="main",
                                                                           seed=9000 + 1000 * ri + 10 * B + K)
        B = 1 if rule == "MSTDPET" else 3
        for shape in ("e1", "e6"):
            out[f"{rule}_b{B}_k3_w_{shape}"] = dict(rule=rule, B=B, K=3, cont=False, shape=shape, seed=9700 + 10 * ri + len(shape))
    out["PostPre_b3_k3_w_post"] = dict(rule="PostPre", B=3, K=3, cont=False, shape="main", seed=9801, nu=(0.0, 0.05))
    out["MSTDP_b3_k3_w_rvec"] = dict(rule="MSTDP", B=3, K=3, cont=False, shape="main", seed=9802, rvec=True)
    return out


CASES = _cases()


def ns_from(nodes, topology, features, mcc_learning, network_cls, monitor_cls):
    return SimpleNamespace(Input=nodes.Input, LIFNodes=nodes.LIFNodes, MulticompartmentConnection=topology.MulticompartmentConnection,
                           Weight=features.Weight, mcc=mcc_learning, Network=network_cls, Monitor=monitor_cls)


def fixture_of(case):
    """The fixture file a case is stored in: one per rule, batch size and mode (every file stays under the size limit)."""
    c = CASES[case]
    return f"mcc_average_{c['rule'].lower()}_b{c['B']}_{'c' if c['cont'] else 'w'}.npz"


def w0(case):
    c = CASES[case]
    return np.random.default_rng(c["seed"] + 1).random(SHAPES[c["shape"]], dtype=np.float32)


def inputs(case, r):
    c = CASES[case]
    s = SHAPES[c["shape"]][0]
    p = 0.3 if c["shape"] == "main" else 0.6
    return (np.random.default_rng(c["seed"] * 10 + r).random((T, c["B"], s)) < p).astype(np.uint8)


def reward(case, r):
    c = CASES[case]
    if c.get("rvec"):
        return torch.from_numpy((REWARDS[r] * np.linspace(-1.0, 1.5, c["B"])).astype(np.float32)).view(-1, 1, 1)   # (against [B, S, N])
    return REWARDS[r]


def build(ns, case, K=None, cont=None, norm=True):
    """The case's network; `K` / `cont` override its average_update / continues_update (K = 0: the plain rule)."""
    c = CASES[case]
    K = c["K"] if K is None else K
    cont = c["cont"] if cont is None else cont
    s, n = SHAPES[c["shape"]]
    main = c["shape"] == "main"
    net = ns.Network(dt=1.0, batch_size=c["B"])
    X = ns.Input(n=s, traces=True, tc_trace=20.0)
    Y = ns.LIFNodes(n=n, traces=True, tc_trace=20.0, thresh=-52.0 if main else -64.6, rest=-65.0, reset=-65.0, refrac=2 if main else 1,
                    tc_decay=100.0)
    feat = ns.Weight("weight", torch.from_numpy(w0(case)), range=[0.0, 1.0], norm=(0.45 * s if norm and main else None),      # (one normalised weight is a constant)
                     nu=[v * min(1.0, 3.0 / c["B"]) for v in c.get("nu", _NU[c["rule"]])],      # (the batch sums grow with B)
                     learning_rule=getattr(ns.mcc, c["rule"]))
    kw = {} if K == 0 else dict(average_update=K, continues_update=cont)
    # (built before add_layer sets the layers' batch size: the rule then reduces over the batch with torch.sum at every B)
    conn = ns.MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat], **kw)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(conn, source="X", target="Y")
    return net


def rule_of(net):
    return net.connections[("X", "Y")].pipeline[0].learning_rule


def weights(net):
    return net.connections[("X", "Y")].pipeline[0].value


def _np(t):
    return t.detach().cpu().numpy().astype(np.float32).copy()


def snapshot(net, case):
    """W, the rings, their indices and the rule's state as numpy arrays."""
    c = CASES[case]
    rule = rule_of(net)
    out = {"w": _np(weights(net))}
    if getattr(rule, "average_update", 0) > 0:
        for ring, index in RINGS[c["rule"]]:
            out[ring] = _np(getattr(rule, ring))
            out[index] = np.int64(getattr(rule, index))
    for name in STATE:
        t = getattr(rule, name, None)
        if isinstance(t, torch.Tensor) and c["rule"] != "PostPre":
            out[name] = _np(t).reshape(-1)
    return out


def run_kwargs(case, r):
    c = CASES[case]
    return {} if c["rule"] == "PostPre" else dict(reward=reward(case, r), a_plus=A_PLUS, a_minus=A_MINUS)


def run(ns, net, case, device=None, n_in=INPUTS, split=None, pipelined=False):
    """The case's inputs through net.run with a reset between them; per input the Y raster and snapshot().  `split`: each input as two
    runs of `split` and T - `split` steps (build the network with norm=False: run() normalises behind every call)."""
    import contextlib
    c = CASES[case]
    out = []
    with (net.pipelined() if pipelined else contextlib.nullcontext()):
        for r in range(n_in):
            x = torch.from_numpy(inputs(case, r))
            x = x if device is None else x.to(device)
            kw = run_kwargs(case, r)
            if device is not None and isinstance(kw.get("reward"), torch.Tensor):
                kw["reward"] = kw["reward"].to(device)
            rasters = []
            for lo, hi in ((0, T),) if split is None else ((0, split), (split, T)):
                mon = ns.Monitor(net.layers["Y"], ["s"], time=hi - lo)
                net.add_monitor(mon, name="Y_mon")
                net.run({"X": x[lo:hi]}, time=hi - lo, **kw)
                rasters.append(mon)
                del net.monitors["Y_mon"]
            if pipelined:
                net.sync()
            got = snapshot(net, case)
            got["raster"] = np.concatenate([m.get("s").cpu().numpy().reshape(-1, c["B"], SHAPES[c["shape"]][1]).astype(np.uint8) for m in rasters])
            out.append(got)
            net.reset_state_variables()
    return out


def conditions(case, got, plain, other, pre_norm):
    """What a fixture must show on the reference's own output.  `plain`: the same case with the plain rule; `other`: with the other
    mode; `pre_norm`: input 1 without the norm (the weights as learning and the clamp leave them).  The tiny shapes (one or six
    weights, a handful of spikes) need not differ between the modes or touch a bound."""
    c = CASES[case]
    assert all(g["raster"].sum() > 0 for g in got), f"{case}: the output layer does not spike"
    assert not np.array_equal(got[0]["w"], w0(case)), f"{case}: W does not move"
    for ring, _ in RINGS[c["rule"]]:
        if c.get("nu", (1, 1))[0] == 0.0 and ring.endswith("_pre"):
            assert not got[-1][ring].any(), f"{case}: the pre ring moved without a pre rate"
            continue
        assert got[0][ring].any(), f"{case}: {ring} is zero at the end of input 1"
    if c["K"] > 1 and c["shape"] == "main":
        assert not np.array_equal(got[-1]["w"], plain[-1]["w"]), f"{case}: W equals the plain rule's"
    elif c["K"] > 1:                  # (a handful of weights may all end at a bound: after either input)
        assert any(not np.array_equal(g["w"], p["w"]) for g, p in zip(got, plain)), f"{case}: W equals the plain rule's"
    else:
        assert np.array_equal(got[-1]["w"], plain[-1]["w"]), f"{case}: K = 1 differs from the plain rule"
    if c["shape"] != "main":
        return
    if c["K"] > 1:
        assert not np.array_equal(got[-1]["w"], other[-1]["w"]), f"{case}: the two modes do not differ"
    w = pre_norm[0]["w"]
    assert (w == 0.0).any() or (w == 1.0).any(), f"{case}: no clamp bound binds"


def pack(case, got):
    """{fixture key: array} of one case."""
    out = {}
    for r, g in enumerate(got):
        for key, a in g.items():
            out[f"{case}/{key}{r}"] = np.packbits(a) if key == "raster" else a
    return out


_GOLD = {}


def gold(case, here):
    """The stored arrays of one case as a list of per-input dicts (rasters unpacked)."""
    import os
    c = CASES[case]
    path = os.path.join(here, "golden", fixture_of(case))
    if path not in _GOLD:
        _GOLD[path] = dict(np.load(path))
    n = SHAPES[c["shape"]][1]
    out = []
    for r in range(INPUTS):
        g = {k[len(case) + 1:-1]: v for k, v in _GOLD[path].items() if k.startswith(case + "/") and k.endswith(str(r))}
        g["raster"] = np.unpackbits(g["raster"])[:T * c["B"] * n].reshape(T, c["B"], n)
        out.append(g)
    return out


def assert_same(case, got, want, what=""):
    """Bit for bit: rasters, W, rings, indices, rule state."""
    for r, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), (case, what, sorted(g), sorted(w))
        for key in w:
            a, b = np.asarray(g[key]), np.asarray(w[key])
            assert np.array_equal(a, b), f"{case} {what}: {key} differs after input {r + 1}" + \
                (f" ({int((a != b).sum())} of {a.size} elements, max |d| {np.abs(a - b).max():.3g})" if a.dtype == np.float32 and a.shape == b.shape else "")
