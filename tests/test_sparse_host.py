"""SparseConnection on the HOST: the package's host path (torch's own sparse product, network/host_path.py) pinned bit for bit to
the reference-generated fixtures of tests/golden/make_golden_sparse.py (cases in tests/sparse_cases.py), the constructor's draws and
clamps, the compiled device form of `w` (ops.sparse_compile, pure torch), what the class refuses, and that a changed `w` is seen."""
import numpy as np
import pytest
import torch

import cases
import sparse_cases as SC


def _ns():
    from bindsnet_amd.network import Network, nodes, topology
    return SC.ns_from(nodes, topology, Network)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_snapshots(name, snaps, first=0):
    """Every recorded quantity bit for bit, the generator's position included."""
    g = cases.gold("sparse_" + name)
    for i, s in enumerate(snaps):
        r = first + i
        want = cases.unpack(g[f"r{r}_raster"], s["raster"].shape)
        assert np.array_equal(s["raster"], want), f"case {name} input {r}: Y raster differs ({int(s['raster'].sum())} vs {int(want.sum())} spikes)"
        assert int(want.sum()) > 0, "a fixture without spikes checks nothing"
        for k, v in s.items():
            if k == "raster":
                continue
            if f"r{r}_{k}_sha" in g.files:
                assert SC.sha(v) == str(g[f"r{r}_{k}_sha"]), f"case {name} input {r}: {k} differs"
            else:
                got, ref = _bits(v).reshape(-1), _bits(g[f"r{r}_{k}"]).reshape(-1)
                assert np.array_equal(got, ref), f"case {name} input {r}: {k} differs at {np.flatnonzero(got != ref)[:5]}"


def _pair(n_src=12, n_dst=7, **kw):
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import SparseConnection
    return SparseConnection(Input(n=n_src, traces=True), LIFNodes(n=n_dst, traces=True), **kw)


def _net(conn, monitor_w=False):
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.monitors import Monitor
    net = Network(dt=1.0)
    net.add_layer(conn.source, name="X")
    net.add_layer(conn.target, name="Y")
    net.add_connection(conn, source="X", target="Y")
    if monitor_w:
        net.add_monitor(Monitor(conn, ["w"], time=3), name="w")
    return net


def _some_w(n_src=12, n_dst=7, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n_src, n_dst, generator=g) * (torch.rand(n_src, n_dst, generator=g) < 0.4)


def test_class_describes_itself():
    from bindsnet.network import topology
    from bindsnet_amd import _lib
    from bindsnet_amd.network.topology import AbstractConnection, Connection, SparseConnection
    assert topology.SparseConnection is SparseConnection and issubclass(SparseConnection, AbstractConnection)
    assert not issubclass(SparseConnection, Connection)         # it takes none of the dense family's rules, masks or modes
    assert SparseConnection._kind == _lib.CONN_SPARSE == 5
    assert SparseConnection._rules == {"NoOp"} and "Connection" in SparseConnection._rules_only
    assert SparseConnection._takes_mask is False and SparseConnection._multi_device is False
    w = _some_w()
    c = _pair(w=w, b=torch.arange(7.0))
    assert isinstance(c.w, torch.nn.Parameter) and c.w.is_sparse and not c.w.requires_grad
    assert torch.equal(c.w.to_dense(), w) and c.w._nnz() == int((w != 0).sum())
    assert torch.equal(c.b, torch.arange(7.0)) and _pair(w=w).b is None
    assert "sp_ptr" not in c.state_dict() and "w" in c.state_dict()


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_construction_draws_the_fixture_weights(name):
    """The constructor's draws (case b: no `w` given, wmin / wmax set) and clamps (case d: wmax on a given `w`)."""
    g = cases.gold("sparse_" + name)
    net = SC.build(_ns(), name)
    assert SC.weights_sha(net) == [str(v) for v in g["w0_sha"]]
    assert [int(c.w._nnz()) for c in net.connections.values()] == g["w0_nnz"].tolist()


def test_constructor_consumes_the_generator_like_connection():
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Connection
    for kw in ({}, dict(wmin=-0.5, wmax=0.25), dict(wmax=0.5)):
        torch.manual_seed(3)
        a = _pair(**kw)
        after = torch.rand(2)
        torch.manual_seed(3)
        b = Connection(Input(n=12), LIFNodes(n=7), **kw)
        assert torch.equal(a.w.to_dense(), b.w) and torch.equal(after, torch.rand(2))


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_host_path_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        net = SC.build(_ns(), name)
        snaps = SC.run_case(net, name, Monitor)
    finally:
        torch.set_num_threads(n)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps)


@pytest.mark.parametrize("shape", [(1, 1), (5, 255), (7, 256), (3, 257), (40, 600), (1100, 37)])
def test_compiled_form_holds_every_entry_in_tile_then_source_then_target_order(shape):
    from bindsnet_amd import _lib, ops
    n_src, n_dst = shape
    g = torch.Generator().manual_seed(n_src + n_dst)
    w = torch.rand(n_src, n_dst, generator=g) * (torch.rand(n_src, n_dst, generator=g) < 0.3)
    ptr, col, val = ops.sparse_compile(w.to_sparse())
    TJ = _lib.SPARSE_TJ
    tiles = (n_dst + TJ - 1) // TJ
    assert ptr.dtype == torch.int32 and col.dtype == torch.uint8 and val.dtype == torch.float32
    assert ptr.numel() == tiles * n_src + 1 and int(ptr[0]) == 0 and int(ptr[-1]) == val.numel() == int((w != 0).sum())
    back = torch.zeros_like(w)
    for t in range(tiles):
        for i in range(n_src):
            lo, hi = int(ptr[t * n_src + i]), int(ptr[t * n_src + i + 1])
            c = col[lo:hi].long()
            assert torch.all(c[1:] > c[:-1]), "targets inside a segment ascend (and are distinct)"
            back[i, t * TJ + c] = val[lo:hi]
    assert torch.equal(back, w)


def test_compiled_form_coalesces_and_keeps_stored_zeros():
    from bindsnet_amd import ops
    idx = torch.tensor([[2, 0, 2, 1], [1, 3, 1, 0]])
    w = torch.sparse_coo_tensor(idx, torch.tensor([1.0, 2.0, 0.5, 0.0]), (3, 4))
    assert not w.is_coalesced()
    ptr, col, val = ops.sparse_compile(w)
    assert ptr.tolist() == [0, 1, 2, 3] and col.tolist() == [3, 0, 1] and val.tolist() == [2.0, 0.0, 1.5]
    with pytest.raises(ValueError):
        ops.sparse_compile(torch.zeros(3, 4))


def test_a_rule_is_refused_with_the_reference_behaviour_named():
    from bindsnet_amd.learning import MSTDP, NoOp, PostPre
    for rule in (PostPre, MSTDP):
        with pytest.raises(NotImplementedError, match="densif|dense learning") as e:
            _pair(update_rule=rule, nu=1e-2)
        assert "SparseConnection" in str(e.value) and "use Connection" in str(e.value)
    assert isinstance(_pair(update_rule=NoOp).update_rule, NoOp)
    with pytest.raises(NotImplementedError, match="Dales_rule"):
        _pair(Dales_rule=torch.ones(12, 7))
    with pytest.raises(NotImplementedError, match="float32"):
        _pair(w_dtype=torch.float64)


def _state(net):
    Y = net.layers["Y"]
    return [t.clone() for t in (Y.v, Y.refrac_count, Y.x, Y.s)] + [torch.get_rng_state()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_norm_mask_monitor_and_dtype_are_refused_before_the_run_changes_anything():
    x = {"X": torch.ones(3, 1, 12, dtype=torch.uint8)}
    w = _some_w() + 5.0
    for make, exc, wording, kwargs in (
            (lambda: _net(_pair(w=w, norm=1.0)), NotImplementedError, r"normalize\(\) raises", {}),
            (lambda: _net(_pair(w=w)), Exception, r"^Mask isn't supported for SparseConnection$",
             {"masks": {("X", "Y"): torch.zeros(12, 7, dtype=torch.bool)}}),
            (lambda: _net(_pair(w=w), monitor_w=True), NotImplementedError, "monitor", {})):
        net = make()
        net.layers["Y"].set_batch_size(1)
        before = _state(net)
        with pytest.raises(exc, match=wording) as e:
            net.run(dict(x), time=3, **kwargs)
        assert type(e.value) is exc and _same(before, _state(net))
    net = _net(_pair(w=w))
    conn = net.connections[("X", "Y")]
    conn.w = torch.nn.Parameter(w.double().to_sparse(), requires_grad=False)
    before = _state(net)
    with pytest.raises(NotImplementedError, match="float32"):
        net.run(dict(x), time=3)
    assert _same(before, _state(net))
    conn.w = torch.nn.Parameter(w, requires_grad=False)          # a dense tensor is not this class's `w`
    with pytest.raises(NotImplementedError, match="sparse COO"):
        net.run(dict(x), time=3)
    # the connection's own methods say the same
    with pytest.raises(Exception, match="^Mask isn't supported for SparseConnection$"):
        _pair(w=w).update(mask=torch.zeros(12, 7, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match=r"normalize\(\) raises"):
        _pair(w=w, norm=2.0).normalize()
    _pair(w=w).normalize()
    _pair(w=w).update(learning=True)
    from bindsnet_amd import parallel
    with pytest.raises(NotImplementedError):
        parallel._refuse(_net(_pair(w=w)), "sharded_run")


def test_changed_weights_are_seen_by_the_next_compute_and_run():
    w = _some_w()
    c = _pair(w=w)
    s = torch.ones(1, 12, dtype=torch.uint8)
    first = c.compute(s)
    assert torch.equal(first, s.float() @ w)
    c.w *= 2                                                   # in place (the values move, the Parameter stays)
    assert torch.equal(c.compute(s), s.float() @ (w * 2))
    c.w._values().mul_(0.5)                                    # in place on the values alone
    assert torch.equal(c.compute(s), first)
    w2 = _some_w(seed=9)
    c.w = torch.nn.Parameter(w2.to_sparse(), requires_grad=False)
    assert torch.equal(c.compute(s), s.float() @ w2)
    # and by run(): the same input leaves Y's voltages elsewhere once the weights are doubled (no neuron reaches its threshold)
    net = _net(_pair(w=0.02 * (w + 0.5)))
    conn = net.connections[("X", "Y")]
    x = torch.ones(20, 1, 12, dtype=torch.uint8)
    net.run({"X": x.clone()}, time=20)
    v1 = net.layers["Y"].v.clone()
    net.reset_state_variables()
    conn.w._values().mul_(2.0)
    net.run({"X": x.clone()}, time=20)
    v2 = net.layers["Y"].v.clone()
    assert torch.all(v2 > v1) and torch.all(v1 > -65.0) and torch.all(v2 < -52.0)


def test_compiled_form_key_follows_every_way_w_changes():
    """The key of the compiled form (which tensor, its in-place version, where values and indices live, device): checked on the
    host, where compiling is pure torch."""
    w = _some_w()
    c = _pair(w=w)

    def dense_of(compiled):
        from bindsnet_amd import _lib
        ptr, col, val = compiled
        out = torch.zeros(12, 7)
        for i in range(12):
            lo, hi = int(ptr[i]), int(ptr[i + 1])
            out[i, col[lo:hi].long()] = val[lo:hi]
        assert _lib.SPARSE_TJ >= 7
        return out

    a = c._compiled()
    assert c._compiled()[2] is a[2], "an unchanged w is compiled once"
    assert torch.equal(dense_of(a), w)
    c.w._values().mul_(3.0)
    assert torch.equal(dense_of(c._compiled()), w * 3.0)
    c.w *= 2
    assert torch.equal(dense_of(c._compiled()), w * 6.0)
    c.w = torch.nn.Parameter(_some_w(seed=11).to_sparse(), requires_grad=False)
    assert torch.equal(dense_of(c._compiled()), _some_w(seed=11))
    c.double().float()                                          # Module._apply re-homes the values behind the same Parameter
    assert torch.equal(dense_of(c._compiled()), _some_w(seed=11))


def test_entry_point_rejects_what_it_cannot_index():
    """Argument checks of snn_prop_sparse_f32 return before anything is launched: no GPU needed."""
    from bindsnet_amd import _lib
    L = _lib.lib()
    assert L.snn_prop_sparse_f32(None, None, None, 0, None, 1, 1, 1, 1, 1, 0, None) == -1
    assert L.snn_prop_sparse_f32(1, None, None, 5, None, 1, 1, 1, 1, 1, 0, None) == -1          # entries without col / val
    assert L.snn_prop_sparse_f32(1, 1, 1, 5, None, 1, 1, 1, (1 << 24) + 1, 1, 0, None) == -2
    assert L.snn_prop_sparse_f32(1, 1, 1, 5, None, 1, 1, 1, 1 << 24, 1 << 16, 0, None) == -2     # 256 tiles x 2^24 sources
    assert L.snn_prop_sparse_f32(1, 1, 1, 5, None, 1, 1, 70000, 8, 8, 0, None) == -2
