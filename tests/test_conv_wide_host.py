"""Conv2dConnection with more than 16 input channels on the HOST: the package's host path (F.conv2d itself) pinned to the
reference-generated fixtures of tests/golden/make_golden_conv_wide.py (cases in tests/conv_wide_cases.py), every field bit for bit;
and what is refused: a learning rule other than NoOp beyond 16 input channels, by name, when the rule is constructed."""
import numpy as np
import pytest
import torch

import cases
import conv_wide_cases as WC


def _ns():
    from bindsnet_amd import conversion
    from bindsnet_amd.network import Network, nodes, topology
    from bindsnet_amd.network.monitors import Monitor
    return WC.ns_from(nodes, topology, Network, Monitor, conversion)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1)


def gold(name):
    return cases.gold("conv_wide_" + name)


def check_snapshots(name, snaps, g, first=0):
    """The snapshots of run_case against the fixture: rasters and every state array bit for bit."""
    seen = spikes = 0
    for i, s in enumerate(snaps):
        r = first + i
        assert {f"r{r}_{k}" for k in s} == {f for f in g.files if f.startswith(f"r{r}_")}
        for k, v in s.items():
            ref = g[f"r{r}_{k}"]
            seen += 1
            if k.endswith("_raster"):
                want = cases.unpack(ref, v.shape)
                assert 0 < int(want.sum()) < want.size, "a raster that is all zeros or all ones checks nothing"
                assert np.array_equal(np.asarray(v, np.uint8), want), f"case {name} input {r}: {k} differs ({int(np.asarray(v).sum())} vs {int(want.sum())} spikes)"
                spikes += int(want.sum())
            else:
                got, want = _bits(v), _bits(ref)
                assert got.size == want.size and np.array_equal(got, want), f"case {name} input {r}: {k} differs at {np.flatnonzero(got != want)[:5]}"
    assert seen > 0 and spikes > 0


def built(name):
    g = gold(name)
    net = WC.build(_ns(), name)
    assert WC.weights_sha(net) == list(g["weights_sha"]), "the initial weights are not the generator's"
    assert WC.wide(net), "no convolution with more than 16 input channels"
    return g, net


@pytest.mark.parametrize("name", WC.NAMES)
def test_host_path_equals_reference(name):
    g, net = built(name)
    snaps = WC.run_case(_ns(), net, name)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps, g)


def test_two_half_runs_equal_one():
    g, net = built("a")
    check_snapshots("a", WC.run_case(_ns(), net, "a", halves=True, count=1), g)


def _conv(cin, rule=None, **kw):
    ns = _ns()
    X, Y = ns.Input(shape=(cin, 5, 5), traces=True), ns.LIFNodes(shape=(4, 3, 3), traces=True)
    if rule is not None:
        kw.update(update_rule=rule, nu=(1e-3, 1e-2))
    return ns.Conv2dConnection(X, Y, kernel_size=3, **kw)


@pytest.mark.parametrize("rule", ["PostPre", "Hebbian", "WeightDependentPostPre", "MSTDP"])
def test_rules_are_refused_beyond_16_input_channels(rule):
    from bindsnet_amd import learning
    kw = dict(wmin=0.0, wmax=1.0) if rule == "WeightDependentPostPre" else {}
    with pytest.raises(NotImplementedError) as e:
        _conv(17, getattr(learning, rule), **kw)
    msg = str(e.value)
    assert rule in msg and "Conv2dConnection" in msg and "17 input channels" in msg and "torch.bmm" in msg
    conn = _conv(17)                                   # the same when the rule is made for an existing connection
    with pytest.raises(NotImplementedError, match="17 input channels"):
        getattr(learning, rule)(connection=conn, nu=(1e-3, 1e-2))
    _conv(16, getattr(learning, rule), **kw)          # 16 channels: as before


def test_postpre_at_16_channels_and_noop_at_17_construct():
    from bindsnet_amd import learning
    assert type(_conv(16, learning.PostPre).update_rule).__name__ == "PostPre"
    assert type(_conv(17).update_rule).__name__ == "NoOp"
    assert type(_conv(17, learning.NoOp).update_rule).__name__ == "NoOp"
    assert _conv(100).w.shape == (4, 100, 3, 3)


def test_other_refusals_stay():
    ns = _ns()
    X, Y = ns.Input(shape=(17, 5, 5)), ns.LIFNodes(shape=(4, 3, 3))
    for kw in (dict(dilation=2), dict(stride=(1, 2)), dict(padding=(0, 1))):
        with pytest.raises(NotImplementedError, match="conv2d supports dilation 1 and symmetric stride/padding only"):
            ns.Conv2dConnection(X, Y, kernel_size=3, **kw)
