"""The per-synapse constant fixture cases (tests/golden/make_golden_synparams.py), written once for both implementations: the
builders take a namespace of classes -- the reference's (the generator) or this package's (the tests).

Op-level cases ("<rule>_b<B>_<variant>"): a dense Connection of S = 37 sources and N = 29 targets whose layer states (s, x) are
SET before each of K consecutive `connection.update()` calls (every bmm has inner dimension 1: the result is order-free), then
`normalize()`.  Recorded after each call: w and the rule's state.  The variants say which constants are tensors and of what shape:

    vec    nu [N] pair         wmin [S, N]   wmax float    norm [N]
    row    nu [1, N] pair      wmin float    wmax [S, 1]   norm [1, N]
    full   nu [S, N] pair      wmin [N]      wmax [S, N]   norm [S, N]   (norm of that shape: host path only)
    col    nu [S, 1] pair      wmin [1, N]   wmax [S, N]   norm [N]

PostPre takes `vec` and `row` only (learning.py:401-402: the others fail in its bmm; synparams_raises.json).  MSTDPET: B = 1.

Run-level cases: Input 40 -> MulticompartmentConnection Weight (tensor range, tensor norm) -> LIF 30 at B = 3 with MCC PostPre /
MSTDP, and Input 40 -> Connection -> LIF 30 with PostPre ([N] rates, [S, N] bounds) / Hebbian ([S, N] rates); 2 inputs x 60 steps.

RAISES: what must fail, and how (type and message recorded from the reference in synparams_raises.json)."""
from types import SimpleNamespace

import numpy as np
import torch

S, N, K = 37, 29, 4
A_PLUS, A_MINUS = 1.0, -0.6           # (the reward-modulated rules: with a_plus == -a_minus the first point eligibility cancels to 0)
RULES = ("PostPre", "Hebbian", "WeightDependentPostPre", "MSTDP", "MSTDPET")
VARIANTS = {
    "vec": dict(nu="N", wmin="SN", wmax=None, norm="N"),
    "row": dict(nu="1N", wmin=None, wmax="S1", norm="1N"),
    "full": dict(nu="SN", wmin="N", wmax="SN", norm="SN"),
    "col": dict(nu="S1", wmin="1N", wmax="SN", norm="N"),
}
_PLAN = {1: ("vec", "row", "full", "col"), 3: ("vec", "full"), 33: ("row", "col")}
_PLAN_POSTPRE = {1: ("vec", "row"), 3: ("vec",), 33: ("row",)}


def op_cases():
    out = {}
    for ri, rule in enumerate(RULES):
        plan = _PLAN_POSTPRE if rule == "PostPre" else _PLAN
        for B, variants in plan.items():
            if rule == "MSTDPET" and B != 1:
                continue
            for vi, v in enumerate(variants):
                out[f"{rule}_b{B}_{v}"] = dict(rule=rule, B=B, variant=v, seed=7000 + 100 * ri + 10 * (B % 7) + vi)
    return out


OP_CASES = op_cases()


def ns_from(nodes, topology, features, learning, mcc_learning, network_cls, monitor_cls):
    return SimpleNamespace(Input=nodes.Input, LIFNodes=nodes.LIFNodes, Connection=topology.Connection,
                           MulticompartmentConnection=topology.MulticompartmentConnection, Weight=features.Weight,
                           learning=learning, mcc=mcc_learning, Network=network_cls, Monitor=monitor_cls)


def _shape(code, s=S, n=N):
    return {"N": (n,), "1N": (1, n), "SN": (s, n), "S1": (s, 1), "1": (1,)}[code]


def _draw(rng, shape, lo, hi):
    return (lo + (hi - lo) * rng.random(shape, dtype=np.float32)).astype(np.float32)


# per rule: the ranges the rates are drawn from (both signs where only that lets a clamp bind on either side), the scalar used where
# a constant stays a float, and the bounds' ranges around initial weights drawn from [0.3, 0.7)
_NU = {"PostPre": (0.02, 0.3), "Hebbian": (-0.3, 0.3), "WeightDependentPostPre": (0.2, 1.5), "MSTDP": (0.02, 0.3), "MSTDPET": (0.5, 6.0)}
_LO, _HI, _WLO, _WHI = (0.15, 0.4), (0.6, 0.85), 0.25, 0.75


def constants(case, mode="tensor"):
    """The case's constants as {nu: (a, b), wmin, wmax, norm}: numpy arrays or floats.  mode "mean": every tensor replaced by the
    float mean of its entries; "uniform": by a tensor of the same shape filled with that mean."""
    c = OP_CASES[case] if case in OP_CASES else RUN_CASES[case]
    v = VARIANTS[c["variant"]] if "variant" in c else c["consts"]
    s, n = c.get("S", S), c.get("N", N)
    rng = np.random.default_rng(c["seed"])
    lo, hi = _NU[c["rule"]]
    out = {}
    nu = None if v["nu"] is None else tuple(_draw(rng, _shape(v["nu"], s, n), lo, hi) for _ in range(2))
    out["nu"] = nu if nu is not None else c.get("nu", (0.5 * (lo + hi), 0.4 * (lo + hi)))
    out["wmin"] = _draw(rng, _shape(v["wmin"], s, n), *_LO) if v["wmin"] else _WLO
    out["wmax"] = _draw(rng, _shape(v["wmax"], s, n), *_HI) if v["wmax"] else _WHI
    out["norm"] = _draw(rng, _shape(v["norm"], s, n), 0.3 * s, 0.6 * s) if v["norm"] else None
    if mode == "tensor":
        return out

    def flat(a):
        if not isinstance(a, np.ndarray):
            return a
        m = np.float32(a.mean())
        return float(m) if mode == "mean" else np.full_like(a, m)
    return {"nu": tuple(flat(a) for a in out["nu"]), "wmin": flat(out["wmin"]), "wmax": flat(out["wmax"]), "norm": flat(out["norm"])}


def _t(a):
    return torch.from_numpy(a.copy()) if isinstance(a, np.ndarray) else a


def w0(case):
    c = OP_CASES[case] if case in OP_CASES else RUN_CASES[case]
    return _draw(np.random.default_rng(c["seed"] + 1), (c.get("S", S), c.get("N", N)), 0.3, 0.7)


def op_states(case):
    """K tuples (s_src bool [B, S], x_src, s_tgt, x_tgt, reward) of numpy arrays."""
    c = OP_CASES[case]
    rng = np.random.default_rng(c["seed"] + 2)
    B = c["B"]
    out = []
    for k in range(K):
        out.append(((rng.random((B, S)) < 0.3), _draw(rng, (B, S), 0.0, 1.5), (rng.random((B, N)) < 0.3), _draw(rng, (B, N), 0.0, 1.5),
                    float((-1.0) ** k * (0.5 + 0.25 * k))))
    return out


def build_op(ns, case, mode="tensor"):
    """Network(batch_size B) with Input S -> Connection (the case's rule and constants) -> LIF N; returns (net, conn)."""
    c = OP_CASES[case]
    k = constants(case, mode)
    net = ns.Network(dt=1.0, batch_size=c["B"])
    X, Y = ns.Input(n=S, traces=True), ns.LIFNodes(n=N, traces=True)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    nu = k["nu"]
    nu = [_t(nu[0]), _t(nu[1])] if isinstance(nu[0], np.ndarray) else (nu[0], nu[1])
    conn = ns.Connection(X, Y, w=torch.from_numpy(w0(case)), wmin=_t(k["wmin"]), wmax=_t(k["wmax"]), norm=_t(k["norm"]),
                         update_rule=getattr(ns.learning, c["rule"]), nu=nu, reduction=torch.sum if c["B"] > 1 else None)
    net.add_connection(conn, source="X", target="Y")
    return net, conn


RULE_STATE = ("p_plus", "p_minus", "eligibility", "eligibility_trace")


def run_op(net, conn, case, device=None, normalize=True):
    """The K update() calls on the set states, then normalize(); returns {f"w{k}", f"{state}{k}", "w_norm"} as numpy arrays, and
    "w_pre" (the weights the normalisation started from)."""
    c = OP_CASES[case]
    X, Y = net.layers["X"], net.layers["Y"]
    out = {}
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).copy()      # noqa: E731
    for k, (ss, xs, st, xt, reward) in enumerate(op_states(case)):
        mv = (lambda a: torch.from_numpy(a)) if device is None else (lambda a: torch.from_numpy(a).to(device))
        X.s, X.x, Y.s, Y.x = mv(ss), mv(xs), mv(st), mv(xt)
        conn.update(reward=reward, a_plus=A_PLUS, a_minus=A_MINUS)
        out[f"w{k}"] = f(conn.w)
        for name in RULE_STATE:
            t = getattr(conn.update_rule, name, None)
            if isinstance(t, torch.Tensor) and not (name == "eligibility" and c["B"] > 3):
                out[f"{name}{k}"] = f(t)
    if normalize:
        conn.normalize()
        out["w_norm"] = f(conn.w)
    return out


def bcast(a, shape=(S, N)):
    return np.broadcast_to(np.asarray(a, np.float32), shape)


def op_conditions(case, got, got_mean):
    """What makes an op-level case a test of anything (asserted by the generator on the reference's output, and again by the host
    test on the fixture): w moves in every call; each bound given as a tensor binds on at least two elements whose bound values
    differ; the result differs from the run with every tensor replaced by its mean; some column's norm / colsum differs from
    norm * (1 / colsum)."""
    k = constants(case)
    prev = w0(case)
    bound_lo = bound_hi = np.zeros((S, N), bool)
    for i in range(K):
        w = got[f"w{i}"]
        assert not np.array_equal(w, prev), f"{case}: call {i} leaves w unchanged"
        bound_lo = bound_lo | (w == bcast(k["wmin"]))
        bound_hi = bound_hi | (w == bcast(k["wmax"]))
        prev = w
    for name, hit in (("wmin", bound_lo), ("wmax", bound_hi)):
        assert hit.sum() >= 2, f"{case}: {name} binds on {hit.sum()} elements"
        if isinstance(k[name], np.ndarray):
            assert len(set(bcast(k[name])[hit].tolist())) >= 2, f"{case}: {name} binds only where it has one value"
    assert not np.array_equal(got[f"w{K - 1}"], got_mean[f"w{K - 1}"]), f"{case}: same result with every tensor replaced by its mean"
    pre = got[f"w{K - 1}"]
    colsum = np.abs(pre).sum(0, dtype=np.float32)
    norm = bcast(k["norm"], (S, N))[0] if np.asarray(k["norm"]).ndim < 2 or np.asarray(k["norm"]).shape[0] == 1 else None
    if norm is not None:
        a, b = norm / colsum, norm * (np.float32(1.0) / colsum)
        assert (a != b).any(), f"{case}: norm / colsum equals norm * (1 / colsum) in every column"


# ---- run-level -------------------------------------------------------------------------------------------------------------------
R_S, R_N, R_T, R_B = 40, 30, 60, 3
RUN_CASES = {
    "mcc_postpre": dict(kind="mcc", rule="PostPre", seed=8101, S=R_S, N=R_N, consts=dict(nu=None, wmin="SN", wmax="N", norm="N"), nu=(0.2, 0.3)),
    "mcc_mstdp": dict(kind="mcc", rule="MSTDP", seed=8102, S=R_S, N=R_N, consts=dict(nu=None, wmin="N", wmax="SN", norm="N"), nu=(0.3, 0.3),
                      reward=0.7),
    "dense_postpre": dict(kind="dense", rule="PostPre", seed=8103, S=R_S, N=R_N, consts=dict(nu="N", wmin="SN", wmax="SN", norm="N")),
    "dense_hebbian": dict(kind="dense", rule="Hebbian", seed=8104, S=R_S, N=R_N, consts=dict(nu="SN", wmin="S1", wmax="1N", norm="N")),
}
_RUN_NU = {"dense_postpre": (0.02, 0.1), "dense_hebbian": (-0.05, 0.05)}
_RUN_SCALE = 0.8           # weights and bounds of the run-level cases are the op-level ones times this (the LIF layer must fire)


def run_constants(case, mode="tensor"):
    c = RUN_CASES[case]
    k = constants(case, mode)
    if case in _RUN_NU and c["consts"]["nu"]:
        lo, hi = _RUN_NU[case]
        rng = np.random.default_rng(c["seed"] + 5)
        nu = tuple(_draw(rng, _shape(c["consts"]["nu"], R_S, R_N), lo, hi) for _ in range(2))
        if mode != "tensor":
            nu = tuple(float(np.float32(a.mean())) if mode == "mean" else np.full_like(a, np.float32(a.mean())) for a in nu)
        k["nu"] = nu
    sc = np.float32(_RUN_SCALE)
    for name in ("wmin", "wmax"):
        k[name] = k[name] * sc if isinstance(k[name], np.ndarray) else float(np.float32(k[name]) * sc)
    if k["norm"] is not None:
        k["norm"] = k["norm"] * sc if isinstance(k["norm"], np.ndarray) else float(np.float32(k["norm"]) * sc)
    return k


def build_run(ns, case, mode="tensor"):
    c = RUN_CASES[case]
    k = run_constants(case, mode)
    torch.manual_seed(c["seed"])
    net = ns.Network(dt=1.0)
    X, Y = ns.Input(n=R_S, traces=True, tc_trace=20.0), ns.LIFNodes(n=R_N, traces=True, tc_trace=20.0, thresh=-52.0, rest=-65.0, reset=-65.0,
                                                                    refrac=5, tc_decay=100.0)
    w = w0(case) * np.float32(_RUN_SCALE)                       # (a Weight asserts that its value starts inside the range)
    w = torch.from_numpy(np.minimum(np.maximum(w, bcast(k["wmin"], w.shape)), bcast(k["wmax"], w.shape)).astype(np.float32))
    if c["kind"] == "mcc":         # (built before add_layer sets a batch size of 1: the rule then reduces over the batch with torch.sum)
        feat = ns.Weight("weight", w, range=[_t(k["wmin"]), _t(k["wmax"])], norm=_t(k["norm"]), nu=list(k["nu"]),
                         learning_rule=getattr(ns.mcc, c["rule"]))
        conn = ns.MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat])
    else:
        nu = [_t(k["nu"][0]), _t(k["nu"][1])] if isinstance(k["nu"][0], np.ndarray) else tuple(k["nu"])
        conn = ns.Connection(X, Y, w=w, wmin=_t(k["wmin"]), wmax=_t(k["wmax"]), norm=_t(k["norm"]), update_rule=getattr(ns.learning, c["rule"]),
                             nu=nu, reduction=torch.sum)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(conn, source="X", target="Y")
    return net


def run_inputs(case, r):
    return (np.random.default_rng(RUN_CASES[case]["seed"] * 10 + r).random((R_T, R_B, R_S)) < 0.25).astype(np.uint8)


def run_weights(net):
    conn = net.connections[("X", "Y")]
    return conn.pipeline[0].value if hasattr(conn, "pipeline") else conn.w


def run_run(ns, net, case, device=None, n_in=2, split=None):
    """The case's inputs through net.run (no reset between them: the weights carry on); per input the Y raster, w after the run
    (normalised) and the target's v.  `split`: each input as two runs of `split` and T - `split` steps."""
    c = RUN_CASES[case]
    kw = {"reward": c["reward"]} if "reward" in c else {}
    out = []
    for r in range(n_in):
        x = torch.from_numpy(run_inputs(case, r))
        x = x if device is None else x.to(device)
        rasters = []
        for lo, hi in ((0, R_T),) if split is None else ((0, split), (split, R_T)):
            mon = ns.Monitor(net.layers["Y"], ["s"], time=hi - lo)
            net.add_monitor(mon, name="Y_mon")
            net.run({"X": x[lo:hi]}, time=hi - lo, **kw)
            rasters.append(mon.get("s").cpu().numpy().reshape(hi - lo, R_B, -1).astype(np.uint8))
            del net.monitors["Y_mon"]
        out.append(dict(raster=np.concatenate(rasters), w=run_weights(net).detach().cpu().numpy().astype(np.float32).copy(),
                        v=net.layers["Y"].v.detach().cpu().numpy().astype(np.float32).copy()))
    return out


def no_norm(net):
    """The network without its normalisation (run() normalises behind every call: two half runs then differ from one whole run)."""
    conn = net.connections[("X", "Y")]
    if hasattr(conn, "pipeline"):
        conn.pipeline[0].norm = None
    else:
        conn.norm = None
    return net


def pre_norm_weights(ns, case):
    """(initial w, w at the end of the case's first input BEFORE run() normalises it): the same run without its norm."""
    net = no_norm(build_run(ns, case))
    start = run_weights(net).detach().cpu().numpy().astype(np.float32).copy()
    return start, run_run(ns, net, case, n_in=1)[0]["w"]


def run_conditions(case, got, got_mean, start, pre):
    """Output spikes; w moves; each clamp binds, on weights that learning moved there, where its bound takes different values; the
    result differs from the run with every tensor replaced by its mean; some column's norm / colsum differs from norm * (1 / colsum).
    `start`, `pre`: pre_norm_weights()."""
    k = run_constants(case)
    shape = pre.shape
    for name in ("wmin", "wmax"):
        hit = (pre == bcast(k[name], shape)) & (pre != start)
        assert hit.sum() >= 2, f"{case}: {name} binds on {hit.sum()} learned elements"
        if isinstance(k[name], np.ndarray):
            assert len(set(bcast(k[name], shape)[hit].tolist())) >= 2, f"{case}: {name} binds only where it has one value"
    colsum = torch.from_numpy(np.abs(pre) if RUN_CASES[case]["kind"] == "dense" else pre).sum(0).numpy()
    norm = np.asarray(k["norm"], np.float32).reshape(-1)
    assert (norm / colsum != norm * (np.float32(1.0) / colsum)).any(), f"{case}: norm / colsum equals norm * (1 / colsum) in every column"
    for r, g in enumerate(got):
        assert g["raster"].sum() >= 50, f"{case} input {r}: only {g['raster'].sum()} output spikes"
        assert 2 * g["raster"].sum() < g["raster"].size, f"{case} input {r}: too many spikes"
        counts = g["raster"].reshape(-1, g["raster"].shape[-1]).sum(0)
        assert len(set(counts.tolist())) >= 3, f"{case} input {r}: the neurons' spike counts hardly differ ({sorted(set(counts.tolist()))})"
    assert not np.array_equal(got[0]["w"], got[1]["w"]), f"{case}: w does not move"
    assert not np.array_equal(got[-1]["w"], got_mean[-1]["w"]), f"{case}: same result with every tensor replaced by its mean"


# ---- what must fail ------------------------------------------------------------------------------------------------------------------
RAISES = {
    "postpre_nu_SN": dict(kind="dense", rule="PostPre", nu="SN", B=1),
    "postpre_nu_S1": dict(kind="dense", rule="PostPre", nu="S1", B=1),
    "postpre_nu_SN_b2": dict(kind="dense", rule="PostPre", nu="SN", B=2),
    "mcc_postpre_nu_SN": dict(kind="mcc", rule="PostPre", nu="SN", B=1),
    "mcc_postpre_nu_N": dict(kind="mcc", rule="PostPre", nu="N", B=1),
    "mcc_mstdp_nu_SN": dict(kind="mcc", rule="MSTDP", nu="SN", B=2),
    "mcc_mstdpet_nu_N": dict(kind="mcc", rule="MSTDPET", nu="N", B=1),
}
X_S, X_N, X_T = 6, 5, 20


def raises_trial(ns, name, device=None):
    """Build the trial's network (6 sources, 5 targets) and run it for 20 steps: returns (net, w before) -- raises what the
    implementation raises, from the constructor or from run()."""
    c = RAISES[name]
    rng = np.random.default_rng(77)
    nu = [torch.from_numpy(_draw(rng, _shape(c["nu"], X_S, X_N), 0.01, 0.1)) for _ in range(2)]
    w = torch.from_numpy(_draw(rng, (X_S, X_N), 0.5, 3.0))
    net = ns.Network(dt=1.0, batch_size=c["B"])
    X, Y = ns.Input(n=X_S, traces=True), ns.LIFNodes(n=X_N, traces=True)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    state = {"net": net, "w": w.clone(), "Y": Y}
    raises_trial.last = state
    if c["kind"] == "mcc":
        feat = ns.Weight("weight", w, range=[0.0, 4.0], nu=nu, learning_rule=getattr(ns.mcc, c["rule"]))
        conn = ns.MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat])
    else:
        conn = ns.Connection(X, Y, w=w, wmin=0.0, wmax=4.0, update_rule=getattr(ns.learning, c["rule"]), nu=nu,
                             reduction=torch.sum if c["B"] > 1 else None)
    net.add_connection(conn, source="X", target="Y")
    state["conn"] = conn
    if device is not None:
        net.to(device)
    x = torch.from_numpy((np.random.default_rng(78).random((X_T, c["B"], X_S)) < 0.5).astype(np.uint8))
    net.run({"X": x if device is None else x.to(device)}, time=X_T, reward=1.0)
    return state
