"""LocalConnection1D / 2D / 3D with PostPre and AdaptiveLIFNodes on the HOST path (plain PyTorch, network/host_path.py), pinned
bit for bit to the reference-generated fixtures of tests/golden/make_golden_local.py (cases in tests/local_cases.py)."""
import numpy as np
import pytest
import torch

import cases
import local_cases as LC


def _ns():
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network, nodes, topology
    return LC.ns_from(nodes, topology, learning, Network)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_snapshots(name, snaps, first=0):
    g = cases.gold("local_" + name)
    c = LC.CASES[name]
    for i, s in enumerate(snaps):
        r = first + i
        want = cases.unpack(g[f"r{r}_raster"], s["raster"].shape)
        assert np.array_equal(s["raster"], want), f"case {name} input {r}: Y raster differs ({int(s['raster'].sum())} vs {int(want.sum())} spikes)"
        for k in ("v", "refrac", "theta", "xX", "xY"):
            got, ref = _bits(s[k]).reshape(-1), _bits(g[f"r{r}_{k}"]).reshape(-1)
            assert np.array_equal(got, ref), f"case {name} input {r}: {k} differs at {np.flatnonzero(got != ref)[:5]}"
        if f"r{r}_w" in g.files:
            got, ref = _bits(s["w"]).reshape(-1), _bits(g[f"r{r}_w"]).reshape(-1)
            assert np.array_equal(got, ref), f"case {name} input {r}: w differs at {np.flatnonzero(got != ref)[:5]}"
        elif r == c["n_in"] - 1 and "final_w" in g.files:
            got, ref = _bits(s["w"]).reshape(-1), _bits(g["final_w"]).reshape(-1)
            assert np.array_equal(got, ref), f"case {name}: final w differs at {np.flatnonzero(got != ref)[:5]}"
        assert LC.sha(s["w"]) == str(g[f"r{r}_w_sha"]), f"case {name} input {r}: w differs"


def test_classes_mirror_the_reference_hierarchy():
    from bindsnet_amd.network.nodes import AdaptiveLIFNodes, DiehlAndCookNodes
    from bindsnet.network import nodes, topology
    assert hasattr(nodes, "AdaptiveLIFNodes") and hasattr(topology, "LocalConnection2D")
    a = AdaptiveLIFNodes(n=4)
    assert not isinstance(a, DiehlAndCookNodes)
    assert not isinstance(DiehlAndCookNodes(n=4), AdaptiveLIFNodes)
    assert float(a.tc_theta_decay) == 1e7 and float(a.theta_plus) == pytest.approx(0.05) and a.theta.shape == (4,)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_construction_draws_the_fixture_weights(name):
    net = LC.build(_ns(), name)
    assert LC.sha(LC.w_of(net).detach().numpy()) == str(cases.gold("local_" + name)["w0_sha"])


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_host_path_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        net = LC.build(_ns(), name)
        snaps = LC.run_case(net, name, Monitor)
    finally:
        torch.set_num_threads(n)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps)


def test_src_table_matches_the_unfolds():
    """src[ci, o, k] is what the reference's unfold chain gathers: check it against explicit index arithmetic in 2D."""
    from bindsnet_amd.network.nodes import AdaptiveLIFNodes, Input
    from bindsnet_amd.network.topology import LocalConnection2D
    X = Input(shape=[2, 9, 11])
    Y = AdaptiveLIFNodes(shape=[3, 3, 3])
    c = LocalConnection2D(X, Y, kernel_size=(4, 3), stride=(2, 3), n_filters=3)
    assert c.src.dtype == torch.int32 and tuple(c.src.shape) == (2, 9, 12)
    for ci in range(2):
        for oy in range(3):
            for ox in range(3):
                for ky in range(4):
                    for kx in range(3):
                        assert int(c.src[ci, oy * 3 + ox, ky * 3 + kx]) == ci * 99 + (oy * 2 + ky) * 11 + ox * 3 + kx


def test_unsupported_rules_and_options_raise():
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import AdaptiveLIFNodes, Input
    from bindsnet_amd.network.topology import LocalConnection1D, LocalConnection2D, LocalConnection3D
    for cls, shape, tshape in ((LocalConnection1D, [1, 8], [2, 3]), (LocalConnection2D, [1, 8, 8], [2, 3, 3]),
                               (LocalConnection3D, [1, 8, 8, 8], [2, 3, 3, 3])):
        for rule in (learning.Hebbian, learning.WeightDependentPostPre, learning.MSTDP, learning.MSTDPET):
            X, Y = Input(shape=shape, traces=True), AdaptiveLIFNodes(shape=tshape, traces=True)
            with pytest.raises(NotImplementedError, match=f"{rule.__name__} on {cls.__name__}"):
                cls(X, Y, kernel_size=4, stride=2, n_filters=2, nu=0.1, update_rule=rule, wmin=0.0, wmax=1.0)
    X, Y = Input(shape=[1, 8, 8], traces=True), AdaptiveLIFNodes(shape=[2, 3, 3], traces=True)
    with pytest.raises(AssertionError):
        LocalConnection2D(X, Y, kernel_size=4, stride=2, n_filters=2, w=torch.rand(2, 3, 3))
    c = LocalConnection2D(X, Y, kernel_size=4, stride=2, n_filters=2, w=torch.full((1, 18, 16), 2.0), wmax=1.0)
    assert float(c.w.max()) == 1.0
    from bindsnet_amd import parallel
    net = Network()
    net.add_layer(X, "X"); net.add_layer(Y, "Y"); net.add_connection(c, "X", "Y")
    with pytest.raises(NotImplementedError, match="LocalConnection2D"):
        parallel.column_shard(net, 0, 2)
    with pytest.raises(NotImplementedError, match="LocalConnection2D"):
        parallel.sharded_run(net, {"X": torch.zeros(2, 1, 1, 8, 8, dtype=torch.uint8)}, time=2)


def _tile_loop(w, F, k, c, i):
    """The reference's tiling (utils.py:219-278) written out element by element."""
    fs = int(np.ceil(np.sqrt(F)))
    (k1, k2), (c1, c2), (i1, i2) = k, c, i
    w = np.asarray(w, np.float32).reshape(F, c1, c2, k1, k2)
    if c1 == 1 and c2 == 1:
        out = np.zeros((i1 * fs, i2 * fs), np.float32)
        for n in range(F):
            out[(n // fs) * i1:(n // fs + 1) * i1, (n % fs) * i2:(n % fs + 1) * i2] = w[n, 0, 0]
        return out
    out = np.zeros((k1 * fs * c1, k2 * fs * c2), np.float32)
    for n1 in range(c1):
        for n2 in range(c2):
            for f in range(F):
                f1, f2 = divmod(f, fs)
                out[k1 * (n1 * fs + f1):k1 * (n1 * fs + f1 + 1), k2 * (n2 * fs + f2):k2 * (n2 * fs + f2 + 1)] = w[f, n1, n2]
    return out


@pytest.mark.parametrize("F,k,c,i", [(5, (4, 3), (3, 2), (9, 7)), (50, (12, 12), (3, 3), (20, 20)), (4, (6, 6), (1, 1), (6, 6))])
def test_reshape_local_connection_2d_weights(F, k, c, i):
    from bindsnet.utils import reshape_local_connection_2d_weights
    torch.manual_seed(F)
    w = torch.rand(F * c[0] * c[1], k[0] * k[1])
    got = reshape_local_connection_2d_weights(w, F, k, c, i).numpy()
    assert np.array_equal(got, _tile_loop(w.numpy(), F, k, c, i))


def test_plot_local_connection_2d_weights():
    import matplotlib
    matplotlib.use("Agg")
    from bindsnet.analysis.plotting import plot_local_connection_2d_weights
    net = LC.build(_ns(), "a")
    lc = net.connections[("X", "Y")]
    im = plot_local_connection_2d_weights(lc, title="LC")
    assert im.get_array().shape == (8 * 12 * 3, 8 * 12 * 3)
    im2 = plot_local_connection_2d_weights(lc, output_channel=3, im=None)
    assert im2.get_array().shape == (12 * 3, 12 * 3)
