"""McCullochPitts / IFNodes / BoostedLIFNodes / CurrentLIFNodes / IzhikevichNodes on the HOST path (plain PyTorch,
network/host_path.py), pinned bit for bit to the reference-generated fixtures of tests/golden/make_golden_nodes.py (cases in
tests/node_cases.py), and the IzhikevichNodes constructor against the reference's buffers and generator position."""
import numpy as np
import pytest
import torch

import cases
import node_cases as NC


def _ns():
    from bindsnet_amd.learning import MCC_learning
    from bindsnet_amd.network import Network, nodes, topology, topology_features
    return NC.ns_from(nodes, topology, topology_features, MCC_learning, Network)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gold(name):
    return cases.gold("nodes_" + name)


def build(name):
    g = gold(name)
    izh = {k: g[k] for k in NC.IZH_BUFFERS} if NC.CASES[name]["kind"] == "izh" else None
    return NC.build(_ns(), name, izh)


def check_snapshots(name, snaps, first=0):
    """Every snapshot against the fixture: raster, per-step v record, every state tensor the layer has, Input trace, weights."""
    g = gold(name)
    for i, s in enumerate(snaps):
        r = first + i
        want = cases.unpack(g[f"r{r}_raster"], s["raster"].shape)
        assert np.array_equal(s["raster"], want), f"case {name} input {r}: Y raster differs ({int(s['raster'].sum())} vs {int(want.sum())} spikes)"
        if f"r{r}_vrec" in g.files:
            got, ref = _bits(s["vrec"]).reshape(-1), _bits(g[f"r{r}_vrec"]).reshape(-1)
            assert np.array_equal(got, ref), f"case {name} input {r}: v record differs at {np.flatnonzero(got != ref)[:5]}"
        assert NC.sha(s["vrec"]) == str(g[f"r{r}_vrec_sha"]), f"case {name} input {r}: v record differs"
        stored = [k for k in NC.STATE + ("xX", "w") if f"r{r}_{k}" in g.files]
        assert set(stored) == set(k for k in s if k not in ("raster", "vrec")), f"case {name}: state tensors {sorted(s)} vs fixture {stored}"
        for k in stored:
            got, ref = _bits(s[k]).reshape(-1), _bits(g[f"r{r}_{k}"]).reshape(-1)
            assert np.array_equal(got, ref), f"case {name} input {r}: {k} differs at {np.flatnonzero(got != ref)[:5]}"


def test_classes_import_from_both_names():
    from bindsnet_amd.network.nodes import BoostedLIFNodes, CurrentLIFNodes, IFNodes, IzhikevichNodes, McCullochPitts
    from bindsnet.network.nodes import Input, IzhikevichNodes as Izh2      # the first import of examples/breakout/breakout.py
    from bindsnet.network import nodes
    assert Izh2 is IzhikevichNodes and Input is nodes.Input
    for cls in (McCullochPitts, IFNodes, BoostedLIFNodes, CurrentLIFNodes, IzhikevichNodes):
        assert getattr(nodes, cls.__name__) is cls
    torch.manual_seed(0)
    m, f, b, c, z = McCullochPitts(n=3), IFNodes(n=3), BoostedLIFNodes(n=3), CurrentLIFNodes(n=3), IzhikevichNodes(n=3)
    assert float(m.thresh) == 1.0 and float(f.reset) == -65.0 and float(b.thresh) == 13.0 and float(c.tc_i_decay) == 2.0
    assert b.refrac_count.dtype == torch.int64 and b.refrac_count.dim() == 0          # an integer scalar until set_batch_size()
    b.set_batch_size(2)
    assert b.refrac_count.dtype == torch.float32 and tuple(b.refrac_count.shape) == (2, 3)
    assert float(z.thresh) == 45.0 and tuple(z.S.shape) == (3, 3) and tuple(z.u.shape) == (3,)
    z.set_batch_size(2)
    assert tuple(z.u.shape) == (2, 3) and torch.equal(z.u, z.b * z.v)
    with pytest.raises(TypeError):
        IzhikevichNodes(shape=[3])
    with pytest.raises(NotImplementedError):
        IFNodes(n=3, sum_input=True)


@pytest.mark.parametrize("seed,n,exc", NC.CTOR)
def test_izhikevich_constructor_matches_the_reference(seed, n, exc):
    from bindsnet_amd.network.nodes import IzhikevichNodes
    g = cases.gold("nodes_ctor")
    torch.manual_seed(seed)
    layer = IzhikevichNodes(n=n, excitatory=exc)
    assert torch.equal(torch.get_rng_state(), torch.from_numpy(g[f"s{seed}_rng"])), "the constructor leaves the generator elsewhere"
    for k in NC.IZH_BUFFERS + ("v", "u"):
        got, ref = getattr(layer, k).numpy(), g[f"s{seed}_{k}"]
        assert got.dtype == ref.dtype and got.shape == ref.shape, k
        assert got.tobytes() == ref.tobytes(), f"buffer {k} differs"
    assert [k for k, _ in layer.named_buffers()][-11:] == ["rest", "thresh", "r", "a", "b", "c", "d", "S", "excitatory", "v", "u"]


@pytest.mark.parametrize("name", sorted(NC.CASES))
def test_host_path_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        net = build(name)
        if NC.CASES[name]["graph"] == "mcc":
            assert NC.sha(NC.weights(net).detach().numpy()) == str(gold(name)["w0_sha"])
        snaps = NC.run_case(net, name, Monitor)
    finally:
        torch.set_num_threads(n)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps)


@pytest.mark.parametrize("name", ["if_b4", "clif_mcc", "izh_mix_b4"])
def test_host_path_at_the_default_thread_count(name):
    """The fixtures are generated at one thread; the host path gives the same bits at whatever count the caller runs."""
    from bindsnet_amd.network.monitors import Monitor
    net = build(name)
    check_snapshots(name, NC.run_case(net, name, Monitor))


def test_standalone_forward_equals_a_run_step():
    """layer.forward(x) on the host is the step Network.run takes."""
    from bindsnet_amd.network.monitors import Monitor
    for name in ("mcp_b4", "if_b4", "boosted_b4", "clif_b4", "izh_mix_b4"):
        c = NC.CASES[name]
        net = build(name)
        snaps = NC.run_case(net, name, Monitor, count=1)
        g = gold(name)
        izh = {k: g[k] for k in NC.IZH_BUFFERS} if c["kind"] == "izh" else None
        Y = NC.make_layer(_ns(), c, izh)
        Y.compute_decays(1.0)
        Y.set_batch_size(c["B"])
        cur = torch.from_numpy(NC.inputs(name, 0)["Y"].copy())
        for t in range(c["T"]):
            Y.forward(cur[t])
            assert np.array_equal(Y.s.numpy().astype(np.uint8), snaps[0]["raster"][t]), (name, t)
        assert np.array_equal(_bits(Y.v.numpy()), _bits(snaps[0]["v"]))


def test_parallel_modes_name_the_layer_type():
    from bindsnet_amd import parallel
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import IFNodes, Input
    from bindsnet_amd.network.topology import Connection
    net = Network()
    X, Y = Input(n=8), IFNodes(n=4)
    net.add_layer(X, "X"); net.add_layer(Y, "Y")
    net.add_connection(Connection(X, Y, w=torch.rand(8, 4)), "X", "Y")
    with pytest.raises(NotImplementedError, match="IFNodes"):
        parallel.column_shard(net, 0, 2)
    with pytest.raises(NotImplementedError, match="IFNodes"):
        parallel.exact_run(net, {"X": torch.zeros(2, 1, 8, dtype=torch.uint8)}, time=2)
