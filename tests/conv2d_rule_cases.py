"""The Conv2dConnection Hebbian / WeightDependentPostPre fixture cases (tests/golden/make_golden_conv2d_rules.py), written once
for both implementations: `build(ns, case)` constructs a case's network from a namespace of classes -- the reference's (the
generator) or this package's (the tests) -- and `run_case` drives it and records, after every input, the Y raster, v,
refrac_count, both traces and w.

Every case keeps OH*OW <= 64: there the reference's torch.bmm adds the output positions in ascending order (checked at L = 64 and
L = 36, batch 1 and 3, 1 and 8 threads), which is the order this package pins; at L = 100 and beyond it does not.

ref_hebbian / ref_wdpp   the shape of the reference's own test/network/test_learning.py: Input [1, 10, 10] -> Conv2dConnection (k 3)
                         -> LIFNodes [32, 8, 8], batch 1
b3_wdpp                  batch 3, 2 input channels, 12 x 12, k 3, stride 2, padding 1, 5 output channels, wmin -0.1, wmax 0.7
                         (w - wmin is not w)
hebb_pre_decay           Hebbian with nu = (1e-3, 0), weight_decay 0.01, wmax 1
wdpp_post_only           WeightDependentPostPre with nu = (0, 1e-2)
hebb_eval                ref_hebbian with network.train(False)"""
import hashlib
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time

CASES = {
    "ref_hebbian": dict(rule="Hebbian", cin=1, hw=(10, 10), k=3, s=1, p=0, cout=32, B=1, T=40, n_in=3, density=0.3, nu=(1e-3, 1e-2),
                        wmin=None, wmax=None, wd=0.0, wscale=0.6, train=True, seed=0),
    "ref_wdpp": dict(rule="WeightDependentPostPre", cin=1, hw=(10, 10), k=3, s=1, p=0, cout=32, B=1, T=40, n_in=3, density=0.3,
                     nu=(1e-3, 1e-2), wmin=0.0, wmax=1.0, wd=0.0, wscale=0.6, train=True, seed=1),
    "b3_wdpp": dict(rule="WeightDependentPostPre", cin=2, hw=(12, 12), k=3, s=2, p=1, cout=5, B=3, T=35, n_in=2, density=0.3,
                    nu=(2e-3, 1e-2), wmin=-0.1, wmax=0.7, wd=0.0, wscale=0.5, train=True, seed=2),
    "hebb_pre_decay": dict(rule="Hebbian", cin=1, hw=(10, 10), k=3, s=1, p=0, cout=6, B=3, T=30, n_in=2, density=0.3, nu=(1e-3, 0.0),
                           wmin=None, wmax=1.0, wd=0.01, wscale=0.8, train=True, seed=3),
    "wdpp_post_only": dict(rule="WeightDependentPostPre", cin=1, hw=(10, 10), k=3, s=1, p=0, cout=6, B=1, T=30, n_in=2, density=0.3,
                           nu=(0.0, 1e-2), wmin=0.0, wmax=1.0, wd=0.0, wscale=0.6, train=True, seed=4),
    "hebb_eval": dict(rule="Hebbian", cin=1, hw=(10, 10), k=3, s=1, p=0, cout=32, B=1, T=40, n_in=2, density=0.3, nu=(1e-3, 1e-2),
                      wmin=None, wmax=None, wd=0.0, wscale=0.6, train=False, seed=0),
}
# b3_wdpp at dt = 0.5 (default 1.0; `time = T * dt` is run): the refractory countdown and the decays of v and both traces, which the
# rule reads.  `sibling`: the dt = 1 case it repeats.
CASES["b3_wdpp_dt05"] = dict(CASES["b3_wdpp"], dt=0.5, T=56, sibling="b3_wdpp")     # (56 steps: three spikes ten steps of refractory period apart)


def ns_from(nodes, topology, learning, network_cls):
    return SimpleNamespace(Input=nodes.Input, LIFNodes=nodes.LIFNodes, Conv2dConnection=topology.Conv2dConnection,
                           Hebbian=learning.Hebbian, WeightDependentPostPre=learning.WeightDependentPostPre, Network=network_cls)


def out_hw(c):
    return tuple((n + 2 * c["p"] - c["k"]) // c["s"] + 1 for n in c["hw"])


def w0_of(name):
    """The case's initial weights: torch.rand after torch.manual_seed(seed), scaled."""
    c = CASES[name]
    torch.manual_seed(c["seed"])
    return c["wscale"] * torch.rand(c["cout"], c["cin"], c["k"], c["k"])


def build(ns, name):
    c = CASES[name]
    net = ns.Network(dt=c.get("dt", 1.0))
    X = ns.Input(shape=[c["cin"], *c["hw"]], traces=True, tc_trace=20.0)
    Y = ns.LIFNodes(shape=[c["cout"], *out_hw(c)], traces=True, tc_trace=20.0)
    kw = dict(kernel_size=c["k"], stride=c["s"], padding=c["p"], nu=c["nu"], update_rule=getattr(ns, c["rule"]), w=w0_of(name),
              weight_decay=c["wd"])
    if c["B"] > 1:
        kw["reduction"] = torch.sum
    for bound in ("wmin", "wmax"):
        if c[bound] is not None:
            kw[bound] = c[bound]
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(ns.Conv2dConnection(X, Y, **kw), source="X", target="Y")
    if not c["train"]:
        net.train(False)
    return net


def inputs(name, r):
    """Input `r` of a case: [T, B, Cin, H, W] uint8, from numpy's generator (same draws everywhere)."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c["seed"] + r + 11)
    return (rng.random((c["T"], c["B"], c["cin"], *c["hw"])) < c["density"]).astype(np.uint8)


def w_of(net):
    return net.connections[("X", "Y")].w


def snapshot(net, raster):
    X, Y = net.layers["X"], net.layers["Y"]
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).copy()      # noqa: E731
    return dict(raster=np.asarray(raster, np.uint8), v=f(Y.v), refrac=f(Y.refrac_count), xX=f(X.x), xY=f(Y.x), w=f(w_of(net)))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(net, name, monitor_cls, device=None):
    """Run the case's inputs (reset_state_variables() between them); returns one snapshot per input."""
    c = CASES[name]
    out = []
    for r in range(c["n_in"]):
        mon = monitor_cls(net.layers["Y"], ["s"], time=c["T"])
        net.add_monitor(mon, name="Y_s")
        x = torch.from_numpy(inputs(name, r))
        if device is not None:
            x = x.to(device)
        net.run({"X": x}, time=run_time(c["T"], c.get("dt", 1.0)))
        raster = mon.get("s").cpu().numpy().reshape(c["T"], c["B"], -1).astype(np.uint8)
        out.append(snapshot(net, raster))
        del net.monitors["Y_s"]
        net.reset_state_variables()
    return out


def gold_path(name):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"conv2d_rules_{name}.npz")


def check_against_gold(snaps, name):
    """Every recorded tensor of every input, bit for bit."""
    g = np.load(gold_path(name))
    c = CASES[name]
    assert len(snaps) == c["n_in"]
    for r, s in enumerate(snaps):
        want = np.unpackbits(g[f"r{r}_raster"])[:s["raster"].size].reshape(s["raster"].shape)
        np.testing.assert_array_equal(s["raster"], want, err_msg=f"{name} input {r}: raster")
        for k in ("v", "refrac", "xX", "xY", "w"):
            np.testing.assert_array_equal(s[k].reshape(-1).view(np.uint32), g[f"r{r}_{k}"].reshape(-1).view(np.uint32),
                                          err_msg=f"{name} input {r}: {k}")
    assert sum(int(s["raster"].sum()) for s in snaps) > 0, "no output spike: vacuous"
    moved = not np.array_equal(snaps[-1]["w"], w0_of(name).numpy())
    assert moved == c["train"], "the weights moved" if moved else "the weights never moved: vacuous"
