"""Hebbian / WeightDependentPostPre on a Conv2dConnection, host path (network/host_path.py: the reference's own torch expressions):
every fixture of tests/golden/conv2d_rules_*.npz -- recorded from the unmodified reference, tests/golden/make_golden_conv2d_rules.py --
bit for bit, and the constructor's contract."""
import numpy as np
import pytest
import torch

import conv2d_rule_cases as CC


def _ns():
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network, nodes, topology
    return CC.ns_from(nodes, topology, learning, Network)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_host_path_reproduces_the_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    net = _ns()
    net = CC.build(net, name)
    snaps = CC.run_case(net, name, Monitor)
    assert net.last_plan == "host-torch"
    CC.check_against_gold(snaps, name)


def _pair(cout=4):
    from bindsnet_amd.network.nodes import Input, LIFNodes
    return Input(shape=[1, 6, 6], traces=True), LIFNodes(shape=[cout, 4, 4], traces=True)


def test_wdpp_without_finite_bounds_asserts():
    from bindsnet_amd.learning import WeightDependentPostPre
    from bindsnet_amd.network.topology import Conv2dConnection
    for kw in (dict(), dict(wmin=0.0), dict(wmax=1.0)):
        with pytest.raises(AssertionError, match="finite wmin and wmax"):
            Conv2dConnection(*_pair(), kernel_size=3, update_rule=WeightDependentPostPre, nu=(1e-3, 1e-2), **kw)
    Conv2dConnection(*_pair(), kernel_size=3, update_rule=WeightDependentPostPre, nu=(1e-3, 1e-2), wmin=0.0, wmax=1.0)


def test_mstdpet_on_conv2d_still_raises():
    from bindsnet_amd.learning import MSTDPET
    from bindsnet_amd.network.topology import Conv2dConnection
    with pytest.raises(NotImplementedError, match="MSTDPET on Conv2dConnection"):
        Conv2dConnection(*_pair(), kernel_size=3, update_rule=MSTDPET, nu=1e-2)


def test_hebbian_with_a_zero_rate_still_adds_and_turns_negative_zero_into_positive_zero():
    """learning.py:1374 / :1378 run whatever the rates are: `w += 0 * post` rewrites a -0.0 weight as +0.0."""
    from bindsnet_amd.learning import Hebbian
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.topology import Conv2dConnection
    X, Y = _pair()
    w = torch.full((4, 1, 3, 3), -0.0)
    w[0] = 5.0                                   # one channel that spikes
    net = Network(dt=1.0)
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(Conv2dConnection(X, Y, kernel_size=3, update_rule=Hebbian, nu=(1e-3, 0.0), w=w), "X", "Y")
    assert np.signbit(net.connections[("X", "Y")].w.numpy()[1:]).all()
    net.run({"X": torch.ones(1, 1, 1, 6, 6, dtype=torch.uint8)}, time=1)
    got = net.connections[("X", "Y")].w.numpy()
    assert (got[1:] == 0).all() and not np.signbit(got[1:]).any()


@pytest.mark.parametrize("name", [n for n, c in CC.CASES.items() if c["train"]])
def test_order_pinned_oracle_helper_reproduces_the_reference_fixture(name):
    """tests/conv_rule_oracle_run.py (what the device plans are compared with beyond OH*OW = 64) against the reference itself, where
    the reference's order is the pinned one."""
    from conv_rule_oracle_run import ConvRuleOracleRun
    c = CC.CASES[name]
    net = CC.build(_ns(), name)
    W, snaps = None, []
    for r in range(c["n_in"]):
        orc = ConvRuleOracleRun(net, c["B"])              # (a fresh state per input: reset_state_variables() between them)
        if W is not None:
            orc.W = W.copy()
        out = orc.run(CC.inputs(name, r))
        W = out["W"]
        snaps.append(dict(raster=out["s"].reshape(c["T"], c["B"], -1), v=out["v"], refrac=out["refrac_count"], xX=out["xX"], xY=out["xY"], w=W))
    CC.check_against_gold(snaps, name)


def test_entry_point_validates_its_arguments_without_a_gpu():
    from bindsnet_amd import _lib
    L = _lib.lib()
    ok = (1, 1, 1, 1, 1, 2, 1, 8, 8, 3, 3, 3, 1, 0, 1e-3, 1e-2)          # W .. x_tgt, B, Cin, H, Wd, Cout, KH, KW, stride, pad, nu0, nu1
    assert L.snn_conv2d_hebbian(None, *ok[1:], 0, 1.0, 0, 0.0, 0, 0.0, 1, None) == -1
    assert L.snn_conv2d_hebbian(*ok, 0, 1.0, 0, 0.0, 0, 0.0, None, None) == -1                # no scratch
    assert L.snn_conv2d_hebbian(*ok[:5], 0, *ok[6:], 0, 1.0, 0, 0.0, 0, 0.0, 1, None) == -1    # B = 0
    assert L.snn_conv2d_hebbian(*ok[:12], 0, *ok[13:], 0, 1.0, 0, 0.0, 0, 0.0, 1, None) == -1  # stride 0
    for has_min, has_max in ((0, 0), (1, 0), (0, 1)):                                          # weight-dependent: both bounds (learning.py:600-602)
        assert L.snn_conv2d_hebbian(*ok, 1, 1.0, has_min, 0.0, has_max, 1.0, 1, None) == -1
