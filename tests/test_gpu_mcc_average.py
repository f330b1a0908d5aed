"""Time-averaged updates (average_update / continues_update) of the MCC rules on the device (snn_postpre_avg_step / snn_mstdp_avg_step /
snn_mstdpet_avg_step, include/snnhip.h f14, and the generic plan of snn_net_run that dispatches them):

  * every fixture case of tests/mcc_average_cases.py (written by the unmodified reference) bit for bit on the generic plan;
  * the three entry points, driven by hand through rule.update(), against the host path at the limits of the launch geometry -- a flat
    pass of 256-thread workgroups, at most 4096 of them: a shape wider and taller than one workgroup, E beyond one grid pass
    (1025 x 1024 > 4096 * 256), K = 256 with a full ring, B = 33;
  * a hand-driven rule.update() sequence equals the same steps inside Network.run; a pipelined section equals synchronous runs;
  * a Monitor on the Weight's value sees the weights change only in due steps when continues_update=False."""
import numpy as np
import pytest
import torch

import mcc_average_cases as AC
from test_mcc_average_host import HERE, ns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", sorted(AC.CASES))
def test_fixture_case_bit_for_bit_on_the_generic_plan(case):
    NS = ns()
    net = AC.build(NS, case)
    net.to(DEV)
    got = AC.run(NS, net, case, device=DEV)
    assert net.last_plan == "generic"
    AC.assert_same(case, got, AC.gold(case, HERE), "device")


# (name, S, N, B, K, continuous, steps, ring prefilled and the index on its last slot)
SWEEP = [("wider_and_taller_than_a_workgroup", 300, 300, 3, 3, False, 4, False),
         ("beyond_one_grid_pass", 1025, 1024, 2, 2, False, 3, False),
         ("k256_windowed_full_ring", 37, 29, 3, 256, False, 2, True),
         ("k256_continuous_full_ring", 37, 29, 3, 256, True, 2, True),
         ("b33", 37, 29, 33, 3, True, 4, False)]


def _op_net(NS, rule, S, N, B, K, cont, w0):
    net = NS.Network(dt=1.0, batch_size=B)
    X, Y = NS.Input(n=S, traces=True), NS.LIFNodes(n=N, traces=True)
    nu = {"PostPre": [0.02, 0.05], "MSTDP": [0.06, 0.0], "MSTDPET": [0.8, 0.0]}[rule]
    feat = NS.Weight("weight", w0.clone(), range=[0.0, 1.0], nu=nu, learning_rule=getattr(NS.mcc, rule))
    conn = NS.MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat], average_update=K, continues_update=cont)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(conn, source="X", target="Y")
    return net


# (MSTDPET is defined for batch size 1: it takes every shape at B = 1 and has no B = 33 cell)
RULE_SWEEP = [(rule,) + s for rule in AC.RULES for s in SWEEP if not (rule == "MSTDPET" and s[0] == "b33")]


@pytest.mark.parametrize("rule,name,S,N,B,K,cont,steps,prefill", RULE_SWEEP, ids=[f"{s[0]}-{s[1]}" for s in RULE_SWEEP])
def test_entry_points_against_the_host_path(rule, name, S, N, B, K, cont, steps, prefill):
    if rule == "MSTDPET":
        B = 1
    NS = ns()
    g = torch.Generator().manual_seed(len(name) * 1000 + K)
    w0 = torch.rand(S, N, generator=g)
    nets = [_op_net(NS, rule, S, N, B, K, cont, w0), _op_net(NS, rule, S, N, B, K, cont, w0)]
    nets[1].to(DEV)
    if prefill:
        for ring, index in AC.RINGS[rule]:
            fill = torch.randn(K, S, N, generator=g) * 0.05
            for net in nets:
                getattr(AC.rule_of(net), ring).copy_(fill)
                setattr(AC.rule_of(net), index, K - 1)
    for k in range(steps):
        s_src, s_tgt = torch.rand(B, S, generator=g) < 0.3, torch.rand(B, N, generator=g) < 0.3
        x_src, x_tgt = torch.rand(B, S, generator=g) * 1.5, torch.rand(B, N, generator=g) * 1.5
        kw = {} if rule == "PostPre" else dict(reward=(-1.0) ** k * (0.5 + 0.25 * k), a_plus=AC.A_PLUS, a_minus=AC.A_MINUS)
        for net, dev in zip(nets, ("cpu", DEV)):
            X, Y = net.layers["X"], net.layers["Y"]
            X.s, X.x, Y.s, Y.x = s_src.to(dev), x_src.to(dev), s_tgt.to(dev), x_tgt.to(dev)
            net.connections[("X", "Y")].update(learning=True, **kw)
        host, dev = (AC.snapshot(net, f"{rule}_b1_k1_w") for net in nets)
        assert sorted(host) == sorted(dev)
        for key in host:
            assert np.array_equal(host[key], dev[key]), f"{rule} {name}: {key} differs after step {k + 1}"
    assert not torch.equal(AC.weights(nets[0]), w0)


@pytest.mark.parametrize("case", ("PostPre_b3_k7_w", "MSTDP_b3_k3_c", "MSTDPET_b1_k7_w"))
def test_hand_driven_updates_equal_network_run(case):
    NS = ns()
    c = AC.CASES[case]
    whole = AC.build(NS, case, norm=False)
    whole.to(DEV)
    want = AC.run(NS, whole, case, device=DEV, n_in=1)[0]
    net = AC.build(NS, case, norm=False)
    net.to(DEV)
    x = torch.from_numpy(AC.inputs(case, 0)).to(DEV)
    conn = net.connections[("X", "Y")]
    for t in range(AC.T):
        net.train(False)                               # the layers step, nothing learns ...
        net.run({"X": x[t:t + 1]}, time=1, **AC.run_kwargs(case, 0))
        net.train(True)
        conn.update(learning=True, **AC.run_kwargs(case, 0))       # ... then the rule, by hand
    got = AC.snapshot(net, case)
    for key in got:
        assert np.array_equal(got[key], want[key]), f"{case}: {key}"
    for _, index in AC.RINGS[c["rule"]]:
        assert int(got[index]) == AC.T % c["K"]


@pytest.mark.parametrize("case", ("PostPre_b3_k7_w", "PostPre_b33_k33_c", "MSTDP_b3_k3_w_rvec", "MSTDPET_b1_k7_c"))
def test_pipelined_section_equals_synchronous_runs(case):
    NS = ns()
    net = AC.build(NS, case)
    net.to(DEV)
    AC.assert_same(case, AC.run(NS, net, case, device=DEV, pipelined=True), AC.gold(case, HERE), "pipelined")


def test_learned_weight_inside_a_longer_pipeline():
    """[Mask, Weight + PostPre with average_update]: the rule, its rings and the norm are those of the Weight, as without averaging."""
    NS = ns()
    from bindsnet_amd.network.topology_features import Mask
    case = "PostPre_b3_k7_w"
    g = torch.Generator().manual_seed(5)
    keep = torch.rand(AC.S, AC.N, generator=g) < 0.8
    outs = []
    for dev in (None, DEV):
        net = AC.build(NS, case)
        old = net.connections[("X", "Y")]
        feat = NS.Weight("weight", torch.from_numpy(AC.w0(case)), range=[0.0, 1.0], norm=0.45 * AC.S, nu=[0.02, 0.05],
                         learning_rule=NS.mcc.PostPre)
        conn = NS.MulticompartmentConnection(old.source, old.target, device="cpu", pipeline=[Mask("mask", keep.clone()), feat],
                                             average_update=7, continues_update=False)
        net.add_connection(conn, source="X", target="Y")
        if dev:
            net.to(dev)
        x = torch.from_numpy(AC.inputs(case, 0))
        mon = NS.Monitor(net.layers["Y"], ["s"], time=AC.T)
        net.add_monitor(mon, name="Y_mon")
        net.run({"X": x if dev is None else x.to(dev)}, time=AC.T)
        rule = feat.learning_rule
        outs.append((mon.get("s").cpu().numpy(), feat.value.detach().cpu().numpy(), rule.average_buffer_pre.cpu().numpy(),
                     rule.average_buffer_post.cpu().numpy(), rule.average_buffer_index_pre, rule.average_buffer_index_post))
        if dev:
            assert net.last_plan == "generic"
    assert outs[0][0].sum() > 0 and outs[0][2].any() and outs[0][4] == AC.T % 7
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", ("PostPre_b3_k7_w", "MSTDP_b3_k7_w"))
def test_weight_monitor_sees_changes_only_in_due_steps(case):
    NS = ns()
    K = AC.CASES[case]["K"]
    recs = []
    for dev in (None, DEV):
        net = AC.build(NS, case, norm=False)
        if dev:
            net.to(dev)
        feat = net.connections[("X", "Y")].pipeline[0]
        mon = NS.Monitor(feat, ["value"], time=AC.T)
        net.add_monitor(mon, name="value")
        x = torch.from_numpy(AC.inputs(case, 0))
        net.run({"X": x if dev is None else x.to(dev)}, time=AC.T, **AC.run_kwargs(case, 0))
        recs.append(mon.get("value").cpu().numpy().reshape(AC.T, *AC.SHAPES["main"]))
    host, dev = recs
    assert np.array_equal(host, dev)
    prev = AC.w0(case)
    changed = []
    for t in range(AC.T):
        changed.append(not np.array_equal(dev[t], prev))
        prev = dev[t]
    assert changed == [(t + 1) % K == 0 for t in range(AC.T)]     # (both cases' output layers spike within the first window)
