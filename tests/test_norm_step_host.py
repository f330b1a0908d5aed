"""Weight(norm_frequency="time step") on the package's host path (network/host_path.py) against the fixtures the unmodified reference
wrote (tests/golden/make_golden_norm_step.py, cases in tests/norm_step_cases.py):

  * every fixture case bit for bit: rasters, layer state, feature values, rule state, generator state after every input;
  * normalize() of the feature, of the connection and at the end of run() is a no-op in this mode; a weight monitor records the
    value each step leaves behind;
  * an unknown string still raises; the half-precision and multi-device refusals raise before any state changes;
  * a "sample" Weight describes itself and runs exactly as before (an existing fixture)."""
import os

import numpy as np
import pytest
import torch

import norm_step_cases as NC

HERE = os.path.dirname(os.path.abspath(__file__))


def ns():
    from bindsnet_amd.learning import MCC_learning
    from bindsnet_amd.network import Network, nodes, topology, topology_features
    from bindsnet_amd.network.monitors import Monitor
    return NC.ns_from(nodes, topology, topology_features, MCC_learning, Network, Monitor)


def run_fixture(NS, case, device=None):
    torch.manual_seed(NC.CASES[case]["seed"])
    net = NC.build(NS, case)
    if device is not None:
        net.to(device)
    return net, NC.run(NS, net, case, device=device)


@pytest.mark.parametrize("case", sorted(NC.CASES))
def test_fixture_case_bit_for_bit(case):
    net, got = run_fixture(ns(), case)
    NC.assert_same(case, got, NC.gold(case, HERE), "host path")
    assert net.last_plan == "host-torch"


def test_column_sums_equal_the_norm_without_learning():
    """(c): NoOp, train(False) -- the fixture's own weights sum to the norm, and so do this path's after ONE step."""
    NS = ns()
    net = NC.build(NS, "c")
    feat = NC.weights(net)["X_Y"]
    assert not np.allclose(feat.value.sum(0).numpy(), 4.0, rtol=1e-3)
    net.run({k: torch.from_numpy(v[:1]) for k, v in NC.inputs("c", 0).items()}, time=1)
    assert np.allclose(feat.value.sum(0).numpy(), 4.0, rtol=1e-5)


def test_normalize_is_a_noop_in_this_mode():
    NS = ns()
    net = NC.build(NS, "a")
    conn = net.connections[("X", "Y")]
    feat = NC.weights(net)["X_Y"]
    before = feat.value.detach().clone()
    feat.normalize()
    conn.normalize()
    net.run({"X": torch.zeros(0, 3, 40, dtype=torch.uint8)}, time=0)        # (run() of no step: only its closing normalisation)
    assert torch.equal(feat.value, before)
    twin = NC.build(NS, "a", frequency="sample")
    twin.connections[("X", "Y")].normalize()
    assert not torch.equal(NC.weights(twin)["X_Y"].value, before)


def test_weight_monitor_records_behind_the_update():
    """Monitor(feature, ["value"]) records at the end of each step: the last record is the value the run leaves (nothing normalises
    behind the last update), and it does not sum to the norm."""
    NS = ns()
    net = NC.build(NS, "a")
    feat = NC.weights(net)["X_Y"]
    mon = NS.Monitor(feat, ["value"], time=5)
    net.add_monitor(mon, name="w")
    net.run({"X": torch.from_numpy(NC.inputs("a", 0)["X"][:5])}, time=5)
    rec = mon.get("value")
    assert torch.equal(rec[-1].reshape(40, 12), feat.value.detach())
    assert not torch.equal(rec[0], rec[-1])


def test_unknown_frequency_still_raises():
    from bindsnet_amd.network.topology_features import Weight
    for bad in ("timestep", "step", None, 3):
        with pytest.raises(NotImplementedError, match="outside the accelerated path"):
            Weight("w", torch.rand(4, 3), norm=1.0, norm_frequency=bad)
    assert Weight("w", torch.rand(4, 3), norm=1.0).norm_frequency == "sample"
    assert Weight("w", torch.rand(4, 3), norm_frequency="time step")._norm_step() is False      # norm=None: nothing is normalised


def test_half_precision_is_refused_by_name():
    from bindsnet_amd.network.topology_features import Weight
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match=f"norm_frequency='time step' on a {dtype} Weight"):
            Weight("w", torch.rand(4, 3).to(dtype), value_dtype=dtype, norm=1.0, norm_frequency="time step")
        Weight("w", torch.rand(4, 3).to(dtype), value_dtype=dtype, norm=1.0)       # ("sample" keeps being taken)


def test_multi_device_modes_refuse_before_any_state_changes():
    from bindsnet_amd import parallel
    NS = ns()
    net = NC.build(NS, "b")
    feat = NC.weights(net)["X_Y"]
    w0 = feat.value.detach().clone()
    x = {"X": torch.from_numpy(NC.inputs("b", 0)["X"][:5])}
    for mode, call in (("sharded_run", lambda: parallel.sharded_run(net, x, time=5, **NC.run_kwargs("b", 0))),
                       ("column_shard", lambda: parallel.column_shard(net, 0, 1)),
                       ("exact_run", lambda: parallel.exact_run(net, x, time=5))):
        with pytest.raises(NotImplementedError, match=f"{mode}: .*norm_frequency='time step'"):
            call()
        assert torch.equal(feat.value, w0)
        assert not net.layers["Y"].s.any() and float(net.layers["Y"].x.abs().sum()) == 0.0


def test_sample_weight_runs_as_before():
    """The default mode against a fixture that predates this one: tests/golden mcc_average, a "sample" Weight with a norm and PostPre."""
    import mcc_average_cases as AC
    from test_mcc_average_host import ns as ans
    case = "PostPre_b3_k1_w"
    NS = ans()
    net = AC.build(NS, case)
    assert net.connections[("X", "Y")].pipeline[0].norm_frequency == "sample"
    AC.assert_same(case, AC.run(NS, net, case), AC.gold(case, HERE), "sample mode")
