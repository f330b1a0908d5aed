"""The CSRMNodes fixture cases (tests/golden/make_golden_csrm.py), written once for both implementations, and the STATED ORDER
of the device kernels restated in plain float32 torch on the CPU.

`build(ns, c, seed)` constructs a case's network from a namespace of classes -- the reference's (the generator) or this
package's (the tests); `run_case` drives it and records, after every input, the Y raster, v, theta, last_spikes, the X -> Y
window s_w, both traces and w.  `stated_run(c, seed)` computes the same record without either: it is test code and calls
nothing of the package.

The stated order (include/snnhip.h, "f13"):
  window current  x[b,i,j] (+)= (((0 + W[s1,j]) + W[s2,j]) + ...) (+ bias[j]) over the sources s1 < s2 < ... that spiked in slot i,
                  connections added slot by slot in the network's connection order;
  step            v = v * decay;  res = sum_i resK[i] * x[b,i,j];  ref = sum_i refK[i] * last[b,i,j]  (ascending i from 0.0f,
                  product then add);  v = v + (res + ref);  s = v >= thresh + theta;  theta;  push s;  lbound;  trace.
The learning rules are restated with the reference's own expressions: they read the layer only through s and x, and the
device's rule kernels are pinned to those expressions bit for bit by the tests of the rules themselves.

A case: src (source shape), N, B, T, n_in (inputs, reset_state_variables() between them), kernel, wres / wref, tau, rule, nu,
density, and the switches thresh_vec, lbound, train, second (a 7-neuron second Input with a biased Connection into Y), recurrent
(a Y -> Y Connection), pervec (tensor-valued tc_decay, theta_plus, tc_theta_decay), ext (an external current into Y).

The last bit of exp(-dt / tc) of a TENSOR of time constants belongs to the host that evaluates it, so the `pervec` case takes its
`decay` and `theta_decay` buffers from the fixture (`decays`), in `build` and in `stated_run` alike."""
from types import SimpleNamespace

import numpy as np
import torch

_BASE = dict(src=(12,), N=12, B=1, T=60, n_in=1, kernel="ExponentialKernel", wres=20, wref=10, tau=1, rule=None, nu=None,
             density=0.15, wscale=0.6, thresh_vec=False, lbound=None, train=True, second=False, recurrent=False, reduction=None, pervec=False, ext=False)


def _case(**kw):
    return dict(_BASE, **kw)


CASES = {
    # test/network/test_learning.py:80-97 of the reference: Input 100 -> Connection (PostPre nu 1e-2) -> CSRMNodes 100, 250 steps
    "learn100": _case(src=(100,), N=100, T=250, rule="PostPre", nu=1e-2, density=0.1, wscale=0.3),
    "b3_postpre": _case(src=(20,), N=16, B=3, T=80, rule="PostPre", nu=(1e-2, 2e-2), reduction="sum", wscale=0.5),
    "k_alpha": _case(kernel="AlphaKernel"),
    "k_slayer": _case(kernel="AlphaKernelSLAYER"),
    "k_laplace": _case(kernel="LaplacianKernel"),
    "k_exp": _case(kernel="ExponentialKernel"),
    # (1 / tau) (1 - t / tau) is negative beyond t = tau: a window of 3 slots at tau = 2.5 keeps the kernel excitatory
    "k_tri": _case(kernel="TriangularKernel", tau=2.5, wres=3),
    "win33_1": _case(wres=33, wref=1),
    "win1_10": _case(wres=1, wref=10),
    "tau25": _case(tau=2.5),
    "src2d": _case(src=(5, 6), N=10),
    "two_conns": _case(second=True),
    "recurrent": _case(recurrent=True),
    "thresh_vec": _case(thresh_vec=True),
    "lbound": _case(lbound=-70.0),
    "eval": _case(train=False),
    "two_inputs": _case(n_in=2, T=40, rule="PostPre", nu=1e-2),
    "mstdp": _case(rule="MSTDP", nu=1e-2),
    "hebbian": _case(rule="Hebbian", nu=(1e-3, 2e-3)),
    # tensor-valued tc_decay, theta_plus and tc_theta_decay (nodes.py:1435, :1438, :1453 broadcast an [n] tensor), batch 2
    "pervec": _case(pervec=True, B=2, rule="PostPre", nu=1e-2),
    # an external current [T, 1, n] into the layer: `+=` broadcasts it over the slots of the window (network.py:388-390).  Host only
    "ext_current": _case(ext=True),
}
HOST_ONLY = ("ext_current",)   # what the device path refuses
N2 = 7                       # neurons of the second Input of `second`
MARGIN_FACTOR = 8.0          # every |v - (thresh + theta)| of the reference run is at least this many v_spread of its case
MAX_SEEDS = 32


def ns_from(nodes, topology, learning, network_cls):
    return SimpleNamespace(Input=nodes.Input, CSRMNodes=nodes.CSRMNodes, Connection=topology.Connection, PostPre=learning.PostPre,
                           MSTDP=learning.MSTDP, Hebbian=learning.Hebbian, Network=network_cls, topology=topology, nodes=nodes)


def n_src(c):
    return int(np.prod(c["src"]))


def weights(c, seed):
    """The case's constants, from numpy's generator (the same numbers for every implementation)."""
    rng = np.random.default_rng(7000 + seed)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))       # noqa: E731
    out = {"w": f(c["wscale"] * rng.random((n_src(c), c["N"])))}
    if c["second"]:
        out["w2"], out["b2"] = f(0.4 * rng.random((N2, c["N"]))), f(0.2 * rng.random(c["N"]) - 0.1)
    if c["recurrent"]:
        out["wrec"] = f(-0.5 * rng.random((c["N"], c["N"])))
    if c["thresh_vec"]:
        out["thresh"] = f(-52.0 + 3.0 * rng.random(c["N"]))
    if c["pervec"]:
        out["tc_decay"], out["theta_plus"] = f(50.0 + 100.0 * rng.random(c["N"])), f(0.2 + 0.6 * rng.random(c["N"]))
        out["tc_theta_decay"] = f(100.0 + 200.0 * rng.random(c["N"]))
    return out


def inputs(c, seed, r):
    """Input `r` of a case: {"X": [T, B, *src] uint8 (, "X2": [T, B, 7])}."""
    rng = np.random.default_rng(100000 * seed + 10 * r + 3)
    out = {"X": (rng.random((c["T"], c["B"], *c["src"])) < c["density"]).astype(np.uint8)}
    if c["second"]:
        out["X2"] = (rng.random((c["T"], c["B"], N2)) < 0.2).astype(np.uint8)
    if c["ext"]:
        out["Y"] = (1.5 * rng.random((c["T"], c["B"], c["N"])) - 0.5).astype(np.float32)
    return out


def build(ns, c, seed, dt=1.0, decays=None):
    wt = weights(c, seed)
    net = ns.Network(dt=dt, batch_size=c["B"])
    X = ns.Input(shape=list(c["src"]), traces=True, tc_trace=20.0)
    kw = dict(responseKernel=c["kernel"], res_window_size=c["wres"], ref_window_size=c["wref"], tau=c["tau"])
    if c["thresh_vec"]:
        kw["thresh"] = wt["thresh"].clone()
    if c["lbound"] is not None:
        kw["lbound"] = c["lbound"]
    kw.update(theta_plus=0.5, tc_theta_decay=200.0)
    if c["pervec"]:
        kw.update(tc_decay=wt["tc_decay"].clone(), theta_plus=wt["theta_plus"].clone(), tc_theta_decay=wt["tc_theta_decay"].clone())
    Y = ns.CSRMNodes(n=c["N"], traces=True, tc_trace=20.0, **kw)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    if decays is not None:
        Y.decay, Y.theta_decay = torch.from_numpy(decays[0]).clone(), torch.from_numpy(decays[1]).clone()
    ckw = {}
    if c["rule"]:
        ckw = dict(update_rule=getattr(ns, c["rule"]), nu=c["nu"], wmin=0.0, wmax=1.0)
        if c["reduction"] == "sum":
            ckw["reduction"] = torch.sum
    net.add_connection(ns.Connection(X, Y, w=wt["w"].clone(), **ckw), source="X", target="Y")
    if c["second"]:
        X2 = ns.Input(n=N2, traces=True, tc_trace=20.0)
        net.add_layer(X2, name="X2")
        net.add_connection(ns.Connection(X2, Y, w=wt["w2"].clone(), b=wt["b2"].clone()), source="X2", target="Y")
    if c["recurrent"]:
        net.add_connection(ns.Connection(Y, Y, w=wt["wrec"].clone()), source="Y", target="Y")
    if not c["train"]:
        net.train(False)
    return net


def run_kwargs(c):
    return {"reward": 1.0} if c["rule"] == "MSTDP" else {}


def snapshot(net, raster):
    X, Y, conn = net.layers["X"], net.layers["Y"], net.connections[("X", "Y")]
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).copy()          # noqa: E731
    return dict(raster=np.asarray(raster, np.uint8), v=f(Y.v), theta=f(Y.theta), last=f(Y.last_spikes), s_w=f(conn.s_w), xX=f(X.x),
                xY=f(Y.x), w=f(conn.w))


def run_case(net, c, seed, monitor_cls, device=None, first=0, count=None, halves=False, **run_kw):
    """Run inputs [first, first + count) of the case, reset_state_variables() between them; one snapshot per input.  `halves`:
    every input in two runs of T/2 steps."""
    out = []
    count = c["n_in"] - first if count is None else count
    for r in range(first, first + count):
        T = c["T"]
        mon = monitor_cls(net.layers["Y"], ["s"], time=T)
        net.add_monitor(mon, name="Y_s")
        x = {k: torch.from_numpy(a) for k, a in inputs(c, seed, r).items()}
        if device is not None:
            x = {k: a.to(device) for k, a in x.items()}
        if halves:
            h = T // 2
            net.run({k: a[:h] for k, a in x.items()}, time=h, **run_kwargs(c), **run_kw)
            net.run({k: a[h:] for k, a in x.items()}, time=T - h, **run_kwargs(c), **run_kw)
        else:
            net.run(x, time=T, **run_kwargs(c), **run_kw)
        raster = mon.get("s").cpu().numpy().reshape(T, c["B"], -1).astype(np.uint8)
        out.append(snapshot(net, raster))
        del net.monitors["Y_s"]
        net.reset_state_variables()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The stated order, in plain float32 torch.
# ---------------------------------------------------------------------------------------------------------------------
def kernels(c):
    """resKernel / refKernel with the reference's expressions (nodes.py:1519-1552) at dt = 1."""
    tau, reset_const, dt = torch.tensor(c["tau"]), torch.tensor(50), torch.tensor(1.0)
    t = torch.arange(0, torch.tensor(c["wres"]), dt)
    res = {"AlphaKernel": lambda: (1 / (tau**2)) * t * torch.exp(-t / tau),
           "AlphaKernelSLAYER": lambda: (1 / tau) * t * torch.exp(1 - t / tau),
           "LaplacianKernel": lambda: (1 / (tau * 2)) * torch.exp(-1 * torch.abs(t / tau)),
           "ExponentialKernel": lambda: (1 / tau) * torch.exp(-t / tau),
           "TriangularKernel": lambda: (1 / tau) * (1 - (t / tau))}[c["kernel"]]()
    t2 = torch.arange(0, torch.tensor(c["wref"]), dt)
    ref = -reset_const * torch.exp(-t2 / tau)
    return torch.flip(res, [0]).float(), torch.flip(ref, [0]).float()


def window_currents(x, window, W, bias=None):
    """x [B, Wres, N] (+)= per slot the ascending-source chain of W's rows (+ bias): a silent source adds 0.0, which changes
    nothing, so the chain over ALL sources in ascending order is the chain over the spiking ones."""
    acc = torch.zeros(window.shape[0], window.shape[1], W.shape[1])
    for s in range(W.shape[0]):
        col = window[:, :, s]
        if col.any():
            acc = acc + col.unsqueeze(2) * W[s]
    if bias is not None:
        acc = acc + bias
    return acc if x is None else x + acc


def csrm_step(st, x, resK, refK, p):
    """One step of the layer in the stated order; `st`: v [B, N], theta [N], last [B, Wref, N], xtr [B, N]."""
    v = st["v"] * p["decay"]
    theta = st["theta"] * p["theta_decay"] if p["learning"] else st["theta"]
    res = torch.zeros_like(v)
    for i in range(resK.numel()):
        res = res + resK[i] * x[:, i]
    ref = torch.zeros_like(v)
    for i in range(refK.numel()):
        ref = ref + refK[i] * st["last"][:, i]
    v = v + (res + ref)
    s = v >= p["thresh"] + theta
    if p["learning"]:
        theta = theta + p["theta_plus"] * s.float().sum(0)
    st["last"] = torch.cat((st["last"][:, 1:], s[:, None].float()), 1)
    if p["lbound"] is not None:
        v = torch.where(v < p["lbound"], torch.tensor(p["lbound"]), v)
    st["v"], st["theta"], st["s"] = v, theta, s
    st["xtr"] = _trace(st["xtr"], s, p["trace_decay"])


def _trace(x, s, decay):
    x = x * decay                                             # nodes.py:96-103, traces_additive = False, trace_scale = 1
    return torch.where(s.bool(), torch.tensor(1.0), x)


def _batch_sum(t):
    acc = t[0]
    for b in range(1, t.shape[0]):
        acc = acc + t[b]
    return acc


def _learn(c, W, rule_st, src_s, src_x, tgt_s, tgt_x):
    """The rule of X -> Y with the reference's expressions (learning.py:390-420, :1052-1135, :1504-1574, :87-104)."""
    nu = c["nu"] if isinstance(c["nu"], tuple) else (c["nu"], c["nu"])
    nu = torch.tensor(nu, dtype=torch.float)
    red = (lambda t: t.squeeze(0)) if src_s.shape[0] == 1 else _batch_sum
    ss, sx = src_s.float().unsqueeze(2), src_x.unsqueeze(2)
    ts, tx = tgt_s.float().unsqueeze(1), tgt_x.unsqueeze(1)
    if c["rule"] == "PostPre":
        W = W - red(torch.bmm(ss, tx * nu[0]))
        W = W + red(torch.bmm(sx, ts * nu[1]))
    elif c["rule"] == "Hebbian":
        W = W + nu[0] * red(torch.bmm(ss, tx))
        W = W + nu[1] * red(torch.bmm(sx, ts))
    elif c["rule"] == "MSTDP":
        W = W + nu[0] * red(1.0 * rule_st["elig"])
        rule_st["pp"] = rule_st["pp"] * torch.exp(-1.0 / torch.tensor(20.0)) + torch.tensor(1.0) * src_s.float()
        rule_st["pm"] = rule_st["pm"] * torch.exp(-1.0 / torch.tensor(20.0)) + torch.tensor(-1.0) * tgt_s.float()
        rule_st["elig"] = torch.bmm(rule_st["pp"].unsqueeze(2), ts) + torch.bmm(ss, rule_st["pm"].unsqueeze(1))
    return W.clamp(0.0, 1.0)


def stated_run(c, seed, record_v=False, decays=None, clamp=None, unclamp=None, inject_v=None):
    """The whole case in the stated order: one snapshot per input, like run_case (and `vrec` [T, B, N] when asked).  clamp / unclamp
    (bool [N]) and inject_v (f32 [N]) as Network.run takes them (network.py:398-429): v += inject_v in front of the layer's step,
    s[:, clamp] = 1 and s[:, unclamp] = 0 behind it -- behind the push into last_spikes, in front of the learning rule."""
    wt = weights(c, seed)
    B, N, ns = c["B"], c["N"], n_src(c)
    resK, refK = kernels(c)
    dt = torch.tensor(1.0)
    if c["pervec"]:
        decay, theta_decay, theta_plus = torch.from_numpy(decays[0]), torch.from_numpy(decays[1]), wt["theta_plus"]
    else:
        decay, theta_decay, theta_plus = torch.exp(-dt / torch.tensor(100.0)), torch.exp(-dt / torch.tensor(200.0)), torch.tensor(0.5)
    p = dict(decay=decay, theta_decay=theta_decay, theta_plus=theta_plus,
             thresh=wt["thresh"] if c["thresh_vec"] else torch.tensor(-52.0), lbound=c["lbound"], learning=c["train"],
             trace_decay=torch.exp(-dt / torch.tensor(20.0)))
    W = wt["w"].clone()
    st = dict(v=torch.full((B, N), -65.0), theta=torch.zeros(N), last=torch.zeros(B, c["wref"], N), xtr=torch.zeros(B, N),
              s=torch.zeros(B, N, dtype=torch.bool))
    win = {k: torch.zeros(B, c["wres"], n) for k, n in (("X", ns), ("X2", N2), ("Y", N))}
    xX = torch.zeros(B, ns)
    sX = torch.zeros(B, ns, dtype=torch.bool)
    sX2 = torch.zeros(B, N2, dtype=torch.bool)
    rule_st = dict(pp=torch.zeros(B, ns), pm=torch.zeros(B, N), elig=torch.zeros(B, ns, N))
    out = []
    for r in range(c["n_in"]):
        inp = {k: torch.from_numpy(a) for k, a in inputs(c, seed, r).items()}
        raster, vrec = [], []
        for t in range(c["T"]):
            # network.py:211-250: every connection pushes its source's spikes of the PREVIOUS step and adds its window
            win["X"] = torch.cat((win["X"][:, 1:], sX[:, None].float()), 1)
            x = window_currents(None, win["X"], W)
            if c["second"]:
                win["X2"] = torch.cat((win["X2"][:, 1:], sX2[:, None].float()), 1)
                x = window_currents(x, win["X2"], wt["w2"], wt["b2"])
            if c["recurrent"]:
                win["Y"] = torch.cat((win["Y"][:, 1:], st["s"][:, None].float()), 1)
                x = window_currents(x, win["Y"], wt["wrec"])
            sX = inp["X"][t].reshape(B, ns).bool()
            xX = _trace(xX, sX, p["trace_decay"])
            if c["second"]:
                sX2 = inp["X2"][t].reshape(B, N2).bool()
            if c["ext"]:
                x = x + inp["Y"][t][:, None, :]
            if inject_v is not None:
                st["v"] = st["v"] + inject_v
            csrm_step(st, x, resK, refK, p)
            if clamp is not None:
                st["s"] = st["s"] | clamp
            if unclamp is not None:
                st["s"] = st["s"] & ~unclamp
            if c["rule"] and c["train"]:
                W = _learn(c, W, rule_st, sX, xX, st["s"], st["xtr"])
            raster.append(st["s"].numpy().astype(np.uint8))
            vrec.append(st["v"].numpy().copy())
        snap = dict(raster=np.stack(raster), v=st["v"].numpy().copy(), theta=st["theta"].numpy().copy(), last=st["last"].numpy().copy(),
                    s_w=win["X"].reshape(B, c["wres"], *c["src"]).numpy().copy(), xX=xX.reshape(B, *c["src"]).numpy().copy(),
                    xY=st["xtr"].numpy().copy(), w=W.numpy().copy())
        if record_v:
            snap["vrec"] = np.stack(vrec)
        out.append(snap)
        # reset_state_variables(): v = rest, s = 0, x = 0; theta, last_spikes and the windows stay
        st["v"], st["xtr"], st["s"] = torch.full((B, N), -65.0), torch.zeros(B, N), torch.zeros(B, N, dtype=torch.bool)
        xX, sX, sX2 = torch.zeros(B, ns), torch.zeros(B, ns, dtype=torch.bool), torch.zeros(B, N2, dtype=torch.bool)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Calls that raise: name -> function of the namespace.  The generator stores the reference's exception type of each.
# ---------------------------------------------------------------------------------------------------------------------
def _small(ns, dt=1.0, **kw):
    net = ns.Network(dt=dt)
    X, Y = ns.Input(n=6, traces=True), ns.CSRMNodes(n=5, traces=True, **kw)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(ns.Connection(X, Y, w=0.5 * torch.ones(6, 5)), source="X", target="Y")
    return net


def _spikes(T, B, n=6):
    return torch.from_numpy((np.random.default_rng(5).random((T, B, n)) < 0.3).astype(np.uint8))


def _other_conn(ns):
    net = ns.Network()
    X, Y = ns.Input(n=6, traces=True), ns.CSRMNodes(n=6, traces=True)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(ns.topology.MeanFieldConnection(X, Y), source="X", target="Y")
    net.run({"X": _spikes(3, 1)}, time=3)


def _batch_change(ns):
    net = _small(ns)
    net.run({"X": _spikes(3, 1)}, time=3)
    net.run({"X": _spikes(3, 2)}, time=3)


RAISING = {
    "rectangular": lambda ns: _small(ns, responseKernel="RectangularKernel").run({"X": _spikes(3, 1)}, time=3),
    "unknown_kernel": lambda ns: _small(ns, responseKernel="NoSuchKernel"),
    "dt_half": lambda ns: _small(ns, dt=0.5).run({"X": _spikes(6, 1)}, time=3),
    "float_res_window": lambda ns: _small(ns, res_window_size=20.5).run({"X": _spikes(3, 1)}, time=3),
    "float_ref_window": lambda ns: _small(ns, ref_window_size=10.5),
    "batch_change": _batch_change,
    "other_connection": _other_conn,
}
