"""The batch reductions torch.mean / torch.amax / torch.amin on the device (the *_red entry points, include/snnhip.h f15, and the generic
plan of snn_net_run that dispatches them) against the fixtures the unmodified reference wrote (tests/reduction_cases.py), under the
criteria of tests/test_reduction_host.py:

  * every fixture case through Network.run (generic plan) and every update-level case through connection.update() (the ops.* calls);
  * the dense kernel's other tile widths (batch 64, 128, 256: 128, 64 and 32 columns per workgroup) and more than one workgroup per
    axis, against the host path;
  * plans: a reduction other than sum sends DiehlAndCook2015 and TwoLayerNetwork to the generic plan, assigning torch.sum back returns
    the plan a network built with torch.sum reports;
  * a `reduce` outside the enum is SNN_ERR_INVALID, from an entry point and from snn_net_run."""
import numpy as np
import pytest
import torch

import reduction_cases as RC
from test_reduction_host import HERE, ns, run_tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_fixture_runs_on_the_generic_plan(case):
    NS = ns()
    net = RC.build(NS, case)
    net.to(DEV)
    want, _ = RC.gold(case, HERE)
    got = RC.run(NS, net, case, device=DEV)
    assert net.last_plan == "generic"
    for g, w in zip(got, want):
        assert np.array_equal(g["raster"], w["raster"]), f"{case}: rasters differ"
    RC.assert_same(case, got, want, "device", w_tol=run_tol(case))


@pytest.mark.parametrize("case", sorted(RC.CASES))
def test_fixture_updates_through_the_ops(case):
    net = RC.build(ns(), case)
    net.to(DEV)
    _, want = RC.gold(case, HERE)
    RC.assert_same(case, RC.run_updates(net, case, device=DEV), want, "device, update calls")


def _pair(NS, kind, rule, S, N, B, reduction, w0):
    nets = []
    for _ in range(2):
        net = NS.Network(dt=1.0, batch_size=B)
        X, Y = NS.Input(n=S, traces=True), NS.LIFNodes(n=N, traces=True)
        nu = {"PostPre": [0.002, 0.005], "Hebbian": [0.003, -0.002], "WeightDependentPostPre": [0.03, 0.06], "MSTDP": [0.006, 0.0]}[rule]
        if kind == "mcc":
            feat = NS.Weight("weight", w0.clone(), range=[0.0, 1.0], nu=nu, learning_rule=getattr(NS.mcc, rule), reduction=reduction)
            conn = NS.MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat])
        else:
            conn = NS.Connection(X, Y, w=w0.clone(), wmin=0.0, wmax=1.0, nu=nu, update_rule=getattr(NS.learning, rule), reduction=reduction)
        net.add_layer(X, name="X")
        net.add_layer(Y, name="Y")
        net.add_connection(conn, source="X", target="Y")
        nets.append(net)
    nets[1].to(DEV)
    return nets


# (batch, columns per workgroup of the dense kernel at that batch: its LDS budget decides)
TILES = [(64, 128), (128, 64), (256, 32)]
TILE_CASES = [(kind, rule, B, red) for B, _ in TILES for red in RC.TESTED
              for kind, rule in (("dense", "PostPre"), ("dense", "WeightDependentPostPre"), ("mcc", "MSTDP"))]


@pytest.mark.parametrize("kind,rule,B,red", TILE_CASES, ids=[f"{k}-{r}-b{b}-{d}" for k, r, b, d in TILE_CASES])
def test_dense_tile_widths_against_the_host_path(kind, rule, B, red):
    """37 x 300: three row tiles (16 rows each, the last partial) and, at 32 columns per workgroup, ten column tiles; density 0.1 so
    that most elements skip samples."""
    NS = ns()
    S, N = 37, 300
    g = torch.Generator().manual_seed(B * 7 + len(rule))
    w0 = torch.rand(S, N, generator=g)
    nets = _pair(NS, kind, rule, S, N, B, RC.REDUCTIONS[red], w0)
    case = f"dense_postpre_b3_{red}"                       # (names the reduction for the zero rule of the comparison)
    for k in range(3):
        s_src, s_tgt = torch.rand(B, S, generator=g) < 0.1, torch.rand(B, N, generator=g) < 0.1
        x_src, x_tgt = torch.rand(B, S, generator=g) * 1.5, torch.rand(B, N, generator=g) * 1.5
        kw = dict(reward=(-1.0) ** k * (0.5 + 0.25 * k), a_plus=RC.A_PLUS, a_minus=RC.A_MINUS) if rule == "MSTDP" else {}
        for net, dev in zip(nets, ("cpu", DEV)):
            X, Y = net.layers["X"], net.layers["Y"]
            X.s, X.x, Y.s, Y.x = s_src.to(dev), x_src.to(dev), s_tgt.to(dev), x_tgt.to(dev)
            RC.conn_of(net).update(learning=True, **kw)
        host, dev = (RC._np(RC.weights(net)) for net in nets)
        assert np.array_equal(RC.canon(host, case).view(np.uint32), RC.canon(dev, case).view(np.uint32)), \
            f"{kind} {rule} B={B} {red}: w differs after call {k + 1} ({int((host != dev).sum())} elements)"
    if red != "amin" or rule == "MSTDP":           # (the minimum over this many sparse samples of terms that are never negative is zero)
        assert not torch.equal(RC.weights(nets[0]), w0)


def _dc(reduction, B=3):
    from bindsnet_amd.models import DiehlAndCook2015
    torch.manual_seed(0)
    net = DiehlAndCook2015(n_inpt=64, n_neurons=16, batch_size=B, reduction=reduction, norm=12.8, nu=(1e-3, 1e-2))
    net.to(DEV)
    return net


def _two(reduction, B=3):
    from bindsnet_amd.models import TwoLayerNetwork
    torch.manual_seed(0)
    net = TwoLayerNetwork(64, n_neurons=16, reduction=reduction, norm=12.8, nu=(1e-3, 1e-2))
    net.to(DEV)
    return net


@pytest.mark.parametrize("make", (_dc, _two), ids=("DiehlAndCook2015", "TwoLayerNetwork"))
def test_plans(make):
    x = {"X": (torch.rand(20, 3, 64, generator=torch.Generator().manual_seed(1)) < 0.3).to(torch.uint8).to(DEV)}
    ref = make(torch.sum)
    ref.run(dict(x), time=20)
    assert ref.last_plan != "generic"
    net = make(torch.mean)
    net.run(dict(x), time=20)
    assert net.last_plan == "generic"
    rule = RC.rule_of_conn(net.connections[("X", "Ae")] if ("X", "Ae") in net.connections else net.connections[("X", "Y")])
    assert rule.reduction is torch.mean
    rule.reduction = torch.sum
    net.run(dict(x), time=20)
    assert net.last_plan == ref.last_plan
    rule.reduction = torch.amax                      # ... and the kept run descriptors notice the next assignment too
    net.run(dict(x), time=20)
    assert net.last_plan == "generic"


def test_reduce_outside_the_enum_is_invalid(monkeypatch):
    from bindsnet_amd import _lib, ops
    NS = ns()
    w = torch.full((8, 6), 0.5, device=DEV)
    s_src, s_tgt = torch.ones(2, 8, dtype=torch.uint8, device=DEV), torch.ones(2, 6, dtype=torch.uint8, device=DEV)
    x_src, x_tgt = torch.ones(2, 8, device=DEV), torch.ones(2, 6, device=DEV)
    monkeypatch.setitem(_lib.REDUCE, "mean", 4)
    with pytest.raises(_lib.SnnError, match=r"code -1"):
        ops.stdp_postpre(w, s_src, x_src, s_tgt, x_tgt, 0.1, 0.1, use_dt=False, reduce="mean")
    with pytest.raises(_lib.SnnError, match=r"code -1"):
        ops.stdp_hebbian(w, s_src, x_src, s_tgt, x_tgt, 0.1, 0.1, reduce="mean")
    assert torch.equal(w, torch.full((8, 6), 0.5, device=DEV))
    case = "mcc_postpre_b3_mean"
    net = RC.build(NS, case)
    net.to(DEV)
    w0 = RC.weights(net).detach().clone()
    with pytest.raises(_lib.SnnError, match=r"code -1"):
        net.run({"X": torch.from_numpy(RC.inputs(case, 0)).to(DEV)}, time=RC.T)
    assert torch.equal(RC.weights(net), w0)
