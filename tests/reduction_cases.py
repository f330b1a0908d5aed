"""The batch-reduction fixture cases (tests/golden/make_golden_reduction.py), written once for both implementations: the builders
take a namespace of classes -- the reference's (the generator) or this package's (the tests).

A case is "<base>_<reduction>" with reduction in mean / amax / amin (`torch.sum` is built too, for the generator's conditions).  Every
base is Input -> one learning connection -> LIF, batch B, and is used twice:

    run-level     INPUTS inputs of T = 40 steps through Network.run with reset_state_variables() between them; recorded after every
                  input: the Y raster, W, the rule's state (p_plus, p_minus; the rings and their indices with average_update);
    update-level  UPDATES calls of connection.update() on layer states (s, x) that are SET before each call, from the case's own
                  generator; recorded after every call: W and the rule's state.  (The reward rules use the eligibility of the call
                  before, so the second call is the one that learns.)

Families (shapes are the smallest at which the kernels can go wrong):
    dense / mcc   37 x 29 (E = 1073: both ATen column classes of the batch sum); e1 / e6: 1 x 1 and 2 x 3 (ATen's inner reduction and
                  the 4 <= E <= 7 class, low LIF thresholds so that they spike)
    conv2d        1 x 6 x 6 with 2 filters 3 x 3 (16 output positions: the reference's bmm adds them in ascending order), and 3 channels
    local2d       1 x 6 x 6, kernel 4, stride 2, 2 filters;  conv1d  2 x 12, kernel 3;  conv3d  1 x 4 x 4 x 4, kernel 2, nu[0] == 0
Batches 1, 3 and 33 (two mask words): input density 0.6 at B = 3, so that many elements have an event in every sample and amin is not
trivially zero; 0.3 at B = 33, so that skipped samples occur and the zero the event-driven kernels fold in matters.
Weights: range [0, 1] with a binding bound, plus `norm` where the family has one."""
from types import SimpleNamespace

import numpy as np
import torch

S, N, T, INPUTS, UPDATES = 37, 29, 40, 2, 3
SHAPES = {"main": (37, 29), "e1": (1, 1), "e6": (2, 3)}
REDUCTIONS = {"sum": torch.sum, "mean": torch.mean, "amax": torch.amax, "amin": torch.amin}
TESTED = ("mean", "amax", "amin")
A_PLUS, A_MINUS = 1.0, -0.6           # (with a_plus == -a_minus the first point eligibility cancels to 0)
REWARDS = (-0.6, 0.8)                 # one per input / update call, the first negative; `rvec`: times a per-sample profile
RINGS = {"PostPre": (("average_buffer_pre", "average_buffer_index_pre"), ("average_buffer_post", "average_buffer_index_post")),
         "MSTDP": (("average_buffer", "average_buffer_index"),)}
STATE = ("p_plus", "p_minus")


def _bases():
    d = {}

    def add(name, **kw):
        kw.setdefault("shape", "main")
        kw["seed"] = 12000 + 37 * len(d)
        d[name] = kw

    # Connection (the dense kernel, scalar constants and per-synapse ones)
    add("dense_postpre_b1", family="dense", rule="PostPre", B=1)
    add("dense_postpre_b3", family="dense", rule="PostPre", B=3)
    add("dense_postpre_b33", family="dense", rule="PostPre", B=33)
    add("dense_postpre_post_b3", family="dense", rule="PostPre", B=3, nu=(0.0, 0.01))
    add("dense_postpre_pv_b3", family="dense", rule="PostPre", B=3, pv=True)
    add("dense_postpre_e1_b3", family="dense", rule="PostPre", B=3, shape="e1")
    add("dense_postpre_e6_b3", family="dense", rule="PostPre", B=3, shape="e6")
    add("dense_hebbian_b3", family="dense", rule="Hebbian", B=3)
    add("dense_wdpp_b33", family="dense", rule="WeightDependentPostPre", B=33)
    add("dense_mstdp_b33", family="dense", rule="MSTDP", B=33, nu=(0.07, 0.0))
    add("dense_mstdp_rvec_b3", family="dense", rule="MSTDP", B=3, rvec=True)
    # MulticompartmentConnection Weight, float32
    add("mcc_postpre_b1", family="mcc", rule="PostPre", B=1)
    add("mcc_postpre_b3", family="mcc", rule="PostPre", B=3)
    add("mcc_postpre_b33", family="mcc", rule="PostPre", B=33)
    add("mcc_postpre_e1_b3", family="mcc", rule="PostPre", B=3, shape="e1")
    add("mcc_postpre_e6_b3", family="mcc", rule="PostPre", B=3, shape="e6")
    add("mcc_mstdp_b33", family="mcc", rule="MSTDP", B=33, nu=(0.07, 0.0))
    add("mcc_mstdp_rvec_b3", family="mcc", rule="MSTDP", B=3, rvec=True)
    # ... with average_update = 3, windowed (w) and continuous (c)
    add("mcc_postpre_k3w_b3", family="mcc", rule="PostPre", B=3, K=3, cont=False)
    add("mcc_postpre_k3c_b33", family="mcc", rule="PostPre", B=33, K=3, cont=True)
    add("mcc_mstdp_k3w_b33", family="mcc", rule="MSTDP", B=33, K=3, cont=False, nu=(0.07, 0.0))
    add("mcc_mstdp_k3c_b3", family="mcc", rule="MSTDP", B=3, K=3, cont=True)
    # ... float16 / bfloat16
    add("mcc_postpre_f16_b3", family="mcc", rule="PostPre", B=3, dtype="float16")
    add("mcc_postpre_bf16_b33", family="mcc", rule="PostPre", B=33, dtype="bfloat16")
    # Conv2dConnection: the per-operator kernels
    add("conv2d_postpre_b3", family="conv2d", rule="PostPre", B=3, cin=1)
    add("conv2d_postpre_c3_b33", family="conv2d", rule="PostPre", B=33, cin=3)
    add("conv2d_hebbian_b33", family="conv2d", rule="Hebbian", B=33, cin=1)
    add("conv2d_wdpp_b3", family="conv2d", rule="WeightDependentPostPre", B=3, cin=1)
    # LocalConnection2D, Conv1dConnection, Conv3dConnection: PostPre
    add("local2d_postpre_b3", family="local2d", rule="PostPre", B=3)
    add("local2d_postpre_b33", family="local2d", rule="PostPre", B=33)
    add("conv1d_postpre_b3", family="conv1d", rule="PostPre", B=3)
    add("conv3d_postpre_nu0_b33", family="conv3d", rule="PostPre", B=33, nu=(0.0, 0.004))
    return d


BASES = _bases()
CASES = {f"{b}_{r}": dict(c, base=b, reduction=r) for b, c in BASES.items() for r in TESTED}
FAMILIES = ("dense", "mcc", "conv2d", "local2d", "conv1d", "conv3d")
_NU = {"PostPre": (0.02, 0.05), "Hebbian": (0.03, -0.02), "WeightDependentPostPre": (0.3, 0.6), "MSTDP": (0.006, 0.0)}
_GEOM = {"conv2d": dict(hw=(6, 6), k=3, s=1, p=0, cout=2), "local2d": dict(cin=1, hw=(6, 6), k=4, s=2, F=2),
         "conv1d": dict(cin=2, hw=(12,), k=3, s=1, p=0, cout=3), "conv3d": dict(cin=1, hw=(4, 4, 4), k=2, s=1, p=0, cout=2)}


def ns_from(nodes, topology, features, learning, mcc_learning, network_cls, monitor_cls):
    return SimpleNamespace(Input=nodes.Input, LIFNodes=nodes.LIFNodes, Connection=topology.Connection,
                           MulticompartmentConnection=topology.MulticompartmentConnection, Conv2dConnection=topology.Conv2dConnection,
                           LocalConnection2D=topology.LocalConnection2D, Conv1dConnection=topology.Conv1dConnection,
                           Conv3dConnection=topology.Conv3dConnection, Weight=features.Weight, learning=learning, mcc=mcc_learning,
                           Network=network_cls, Monitor=monitor_cls)


def base_of(case):
    return CASES[case]["base"] if case in CASES else case


def fixture_of(case):
    """One fixture file per family and rule, the averaged and the half-precision MCC cases in files of their own (each in the size range
    of the other fixtures here)."""
    c = BASES[base_of(case)]
    tail = "_avg" if c.get("K") else "_half" if c.get("dtype") else ""
    return f"reduction_{c['family']}_{c['rule'].lower()}{tail}.npz"


def density(c):
    if c["shape"] != "main":
        return 0.8               # (one or six weights: all three samples must spike for a non-zero minimum)
    return 0.6 if c["B"] <= 3 else 0.3


def source_shape(c):
    f = c["family"]
    if f in ("dense", "mcc"):
        return (SHAPES[c["shape"]][0],)
    g = _GEOM[f]
    return (c.get("cin", g.get("cin")), *g["hw"])


def target_shape(c):
    f = c["family"]
    if f in ("dense", "mcc"):
        return (SHAPES[c["shape"]][1],)
    g = _GEOM[f]
    out = tuple((n + 2 * g.get("p", 0) - g["k"]) // g["s"] + 1 for n in g["hw"])
    return (g["cout"], *out) if "cout" in g else (g["F"], *out)


def w0(base):
    """The initial [S, N] weights of a dense / mcc case (the other families draw theirs from torch's generator after manual_seed)."""
    c = BASES[base]
    return np.random.default_rng(c["seed"] + 1).random(SHAPES[c["shape"]], dtype=np.float32)


def nu_of(c):
    nu = c.get("nu", _NU[c["rule"]])
    if c["family"] not in ("dense", "mcc") and "nu" not in c:      # (a convolutional term is a sum over the output positions)
        nu = (0.1 * nu[0], 0.4 * nu[1]) if c["family"] == "local2d" else (0.13 * nu[0], 0.2 * nu[1])
    scale = min(1.0, 3.0 / c["B"])            # (the batch sums grow with B; the same rates for every reduction of a base)
    return [v * scale for v in nu]


def _pv_constants(c):
    rng = np.random.default_rng(c["seed"] + 3)
    s, n = SHAPES[c["shape"]]
    nu = [torch.from_numpy((lo + (hi - lo) * rng.random(n)).astype(np.float32)) for lo, hi in ((0.005, 0.04), (0.01, 0.09))]
    wmin = torch.from_numpy((0.2 * rng.random((s, n))).astype(np.float32))
    wmax = torch.from_numpy((0.8 + 0.2 * rng.random((s, n))).astype(np.float32))
    return nu, wmin, wmax


def build(ns, case, reduction=None, norm=True):
    """The network of a case (or of a base, with `reduction` named).  `norm=False`: without the normalisation (the weights as learning
    and the clamp leave them)."""
    base = base_of(case)
    c = BASES[base]
    red = REDUCTIONS[reduction or CASES[case]["reduction"]]
    f, B = c["family"], c["B"]
    main = c["shape"] == "main"
    net = ns.Network(dt=1.0, batch_size=B)
    torch.manual_seed(c["seed"])
    if f in ("dense", "mcc"):
        s, n = SHAPES[c["shape"]]
        X = ns.Input(n=s, traces=True, tc_trace=20.0)
        Y = ns.LIFNodes(n=n, traces=True, tc_trace=20.0, thresh=-52.0 if main else -64.6, rest=-65.0, reset=-65.0, refrac=2 if main else 1,
                        tc_decay=100.0)
        w = torch.from_numpy(w0(base))
        nrm = 0.45 * s if norm and main else None              # (one normalised weight is a constant)
        if f == "dense":
            kw = dict(w=w, wmin=0.0, wmax=1.0, norm=nrm, update_rule=getattr(ns.learning, c["rule"]), nu=nu_of(c), reduction=red)
            if c.get("pv"):
                kw["nu"], kw["wmin"], kw["wmax"] = _pv_constants(c)
                kw["w"] = torch.minimum(torch.maximum(w, kw["wmin"]), kw["wmax"])
            conn = ns.Connection(X, Y, **kw)
        else:
            dtype = getattr(torch, c.get("dtype", "float32"))
            feat = ns.Weight("weight", w.to(dtype), value_dtype=dtype, range=[0.0, 1.0], norm=nrm, nu=nu_of(c),
                             learning_rule=getattr(ns.mcc, c["rule"]))
            kw = dict(average_update=c["K"], continues_update=c["cont"]) if c.get("K") else {}
            conn = ns.MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat], **kw)
            # (the reference's Weight(..., reduction=f) trips its own assertion, topology_features.py:117-118: the rule reads the
            #  attribute at every update, so assigning it is how a reduction reaches an MCC rule there)
            feat.learning_rule.reduction = red
    else:
        g = _GEOM[f]
        X = ns.Input(shape=list(source_shape(c)), traces=True, tc_trace=20.0)
        Y = ns.LIFNodes(shape=list(target_shape(c)), traces=True, tc_trace=20.0, thresh=-60.0, rest=-65.0, reset=-65.0, refrac=2, tc_decay=100.0)
        kw = dict(kernel_size=g["k"], stride=g["s"], nu=nu_of(c), update_rule=getattr(ns.learning, c["rule"]), wmin=0.0, wmax=1.0, reduction=red)
        if f == "conv2d":
            kw.update(padding=g["p"], w=0.9 * torch.rand(g["cout"], c["cin"], g["k"], g["k"]))
            conn = ns.Conv2dConnection(X, Y, **kw)
        elif f == "local2d":
            conn = ns.LocalConnection2D(X, Y, n_filters=g["F"], norm=(0.4 * g["k"] * g["k"] if norm else None), **kw)
        else:
            conn = (ns.Conv1dConnection if f == "conv1d" else ns.Conv3dConnection)(X, Y, padding=g["p"], **kw)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(conn, source="X", target="Y")
    return net


def conn_of(net):
    return net.connections[("X", "Y")]


def rule_of_conn(conn):
    return conn.pipeline[0].learning_rule if hasattr(conn, "pipeline") else conn.update_rule


def rule_of(net):
    return rule_of_conn(conn_of(net))


def weights(net):
    conn = conn_of(net)
    return conn.pipeline[0].value if hasattr(conn, "pipeline") else conn.w


def inputs(case, r):
    c = BASES[base_of(case)]
    return (np.random.default_rng(c["seed"] * 10 + r).random((T, c["B"], *source_shape(c))) < density(c)).astype(np.uint8)


def reward(case, r):
    c = BASES[base_of(case)]
    if c.get("rvec"):
        return torch.from_numpy((REWARDS[r % 2] * np.linspace(-1.0, 1.5, c["B"])).astype(np.float32)).view(-1, 1, 1)   # (against [B, S, N])
    return REWARDS[r % 2]


def run_kwargs(case, r, device=None):
    c = BASES[base_of(case)]
    if c["rule"] != "MSTDP":
        return {}
    rw = reward(case, r)
    if device is not None and isinstance(rw, torch.Tensor):
        rw = rw.to(device)
    return dict(reward=rw, a_plus=A_PLUS, a_minus=A_MINUS)


def _np(t):
    return t.detach().cpu().float().numpy().astype(np.float32).copy()


def snapshot(net, case):
    """W (a half Weight widened: exact), the rings and their indices, the reward rule's factors."""
    c = BASES[base_of(case)]
    rule = rule_of(net)
    out = {"w": _np(weights(net))}
    if getattr(rule, "average_update", 0) > 0:
        for ring, index in RINGS[c["rule"]]:
            out[ring] = _np(getattr(rule, ring))
            out[index] = np.int64(getattr(rule, index))
    if c["rule"] == "MSTDP":
        for name in STATE:
            t = getattr(rule, name, None)
            if isinstance(t, torch.Tensor):
                out[name] = _np(t).reshape(-1)
    return out


def run(ns, net, case, device=None, n_in=INPUTS):
    """The case's inputs through net.run with a reset between them; per input the Y raster and snapshot()."""
    c = BASES[base_of(case)]
    out = []
    for r in range(n_in):
        x = torch.from_numpy(inputs(case, r))
        x = x if device is None else x.to(device)
        mon = ns.Monitor(net.layers["Y"], ["s"], time=T)
        net.add_monitor(mon, name="Y_mon")
        net.run({"X": x}, time=T, **run_kwargs(case, r, device))
        got = snapshot(net, case)
        got["raster"] = mon.get("s").cpu().numpy().reshape(T, c["B"], -1).astype(np.uint8)
        del net.monitors["Y_mon"]
        out.append(got)
        net.reset_state_variables()
    return out


def update_states(case):
    """UPDATES tuples (s_src bool, x_src, s_tgt bool, x_tgt) of numpy arrays shaped [B, *layer shape]."""
    c = BASES[base_of(case)]
    rng = np.random.default_rng(c["seed"] + 2)
    B, p = c["B"], density(c)
    out = []
    for _ in range(UPDATES):
        out.append((rng.random((B, *source_shape(c))) < p, (1.5 * rng.random((B, *source_shape(c)))).astype(np.float32),
                    rng.random((B, *target_shape(c))) < p, (1.5 * rng.random((B, *target_shape(c)))).astype(np.float32)))
    return out


def run_updates(net, case, device=None, spy=None):
    """UPDATES connection.update() calls on set layer states; per call snapshot().  `spy(k, net)`: called before call k."""
    X, Y, conn = net.layers["X"], net.layers["Y"], conn_of(net)
    mv = (lambda a: torch.from_numpy(a)) if device is None else (lambda a: torch.from_numpy(a).to(device))
    out = []
    for k, (ss, xs, st, xt) in enumerate(update_states(case)):
        X.s, X.x, Y.s, Y.x = mv(ss), mv(xs), mv(st), mv(xt)
        if spy is not None:
            spy(k, net)
        conn.update(learning=True, **run_kwargs(case, k, device))      # (a MulticompartmentConnection learns only when told so)
        out.append(snapshot(net, case))
    return out


def pack(case, runs, updates):
    """{fixture key: array} of one case: "<case>/<key><r>" per input, "<case>/u_<key><k>" per update call."""
    out = {}
    for r, g in enumerate(runs):
        for key, a in g.items():
            out[f"{case}/{key}{r}"] = np.packbits(a) if key == "raster" else a
    for k, g in enumerate(updates):
        for key, a in g.items():
            out[f"{case}/u_{key}{k}"] = a
    return out


_GOLD = {}


def gold(case, here):
    """(runs, updates) of one case from its fixture: lists of per-input / per-call dicts (rasters unpacked)."""
    import os
    c = BASES[base_of(case)]
    path = os.path.join(here, "golden", fixture_of(case))
    if path not in _GOLD:
        _GOLD[path] = dict(np.load(path))
    mine = {k[len(case) + 1:]: v for k, v in _GOLD[path].items() if k.startswith(case + "/")}
    n = int(np.prod(target_shape(c)))
    runs = []
    for r in range(INPUTS):
        g = {k[:-1]: v for k, v in mine.items() if not k.startswith("u_") and k.endswith(str(r))}
        g["raster"] = np.unpackbits(g["raster"])[:T * c["B"] * n].reshape(T, c["B"], n)
        runs.append(g)
    updates = [{k[2:-1]: v for k, v in mine.items() if k.startswith("u_") and k.endswith(str(i))} for i in range(UPDATES)]
    return runs, updates


def canon(a, case):
    """amax / amin: the sign of a zero result is not defined (torch's own differs between its scalar and vector paths), so -0 is
    compared as +0 there; everything else is compared as it is."""
    a = np.asarray(a)
    if a.dtype == np.float32 and CASES[case]["reduction"] in ("amax", "amin"):
        return a + np.float32(0.0)
    return a


def assert_same(case, got, want, what="", w_tol=None):
    """Bit for bit: rasters, W, rings, indices, rule state (zeros canonicalised for amax / amin).  `w_tol`: the weights (and the rings)
    within that margin instead -- the dense Connection's runs, whose propagation is the reference's matmul."""
    for r, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), (case, what, sorted(g), sorted(w))
        for key in w:
            a, b = canon(g[key], case), canon(w[key], case)
            if w_tol is not None and a.dtype == np.float32:
                assert a.shape == b.shape and np.abs(a - b).max(initial=0.0) <= w_tol, \
                    f"{case} {what}: {key} differs after step {r + 1} by {np.abs(a - b).max():.3g} > {w_tol}"
                continue
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                         b.view(np.uint32) if b.dtype == np.float32 else b), \
                f"{case} {what}: {key} differs after step {r + 1}" + \
                (f" ({int((a != b).sum())} of {a.size} elements, max |d| {np.abs(a - b).max():.3g})" if a.dtype == np.float32 and a.shape == b.shape else "")
