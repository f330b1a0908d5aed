"""MaxPool1d / 2d / 3dConnection and MeanFieldConnection on the HOST: the package's host path (torch's own max_pool and mean,
network/host_path.py) pinned bit for bit to the reference-generated fixtures of tests/golden/make_golden_pool.py (cases in
tests/pool_cases.py) at one thread and at the default thread count, compute() by hand, the constructors' draws and clamps, and
everything the classes raise -- where the reference raises too, its recorded exception type; where this package deviates on
purpose (training mode, a connection built before its layers), that it runs."""
import numpy as np
import pytest
import torch

import cases
import pool_cases as PC


def _ns():
    from bindsnet_amd import learning
    from bindsnet_amd.network import Network, nodes, topology
    return PC.ns_from(nodes, topology, Network, learning)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_snapshots(name, snaps, first=0):
    """Every recorded quantity bit for bit."""
    g = cases.gold("pool_" + name)
    for i, s in enumerate(snaps):
        r = first + i
        want = cases.unpack(g[f"r{r}_raster"], s["raster"].shape)
        assert int(want.sum()) > 0, "a fixture without spikes checks nothing"
        assert np.array_equal(s["raster"], want), f"case {name} input {r}: Y raster differs ({int(s['raster'].sum())} vs {int(want.sum())} spikes)"
        for k, v in s.items():
            if k == "raster":
                continue
            got, ref = _bits(v).reshape(-1), _bits(g[f"r{r}_{k}"]).reshape(-1)
            assert got.size == ref.size and np.array_equal(got, ref), f"case {name} input {r}: {k} differs at {np.flatnonzero(got != ref)[:5]}"


def test_reference_names_resolve():
    from bindsnet.network import topology
    from bindsnet_amd import _lib
    from bindsnet_amd.network import topology as own
    for name in ("MaxPool1dConnection", "MaxPool2dConnection", "MaxPoo3dConnection", "MaxPool3dConnection", "MeanFieldConnection"):
        assert getattr(topology, name) is getattr(own, name) and issubclass(getattr(own, name), own.AbstractConnection)
    assert own.MaxPool3dConnection is own.MaxPoo3dConnection
    assert own.MaxPool2dConnection._kind == _lib.CONN_POOL == 6 and own.MeanFieldConnection._kind == _lib.CONN_MEANFIELD == 7
    for cls in (own.MaxPool1dConnection, own.MaxPool2dConnection, own.MaxPoo3dConnection, own.MeanFieldConnection):
        assert cls._rules == {"NoOp"} and cls._takes_mask is False and cls._multi_device is False


def test_fixtures_decide_the_index_rule():
    """What the generator measured: in every pooling fixture at least a tenth of the window decisions picked a tap other than the
    window's first in-bounds one, and ties occurred."""
    for name in sorted(PC.POOL) + ["h"] + sorted(PC.DT):
        g = cases.gold("pool_" + name)
        assert float(g["share_nonfirst"]) >= 0.10 and float(g["share_ties"]) > 0.0, name


@pytest.mark.parametrize("threads", [1, None])
@pytest.mark.parametrize("name", PC.CASES)
def test_host_path_reproduces_reference_fixture(name, threads):
    from bindsnet_amd.network.monitors import Monitor
    n = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        net = PC.build(_ns(), name)
        for key, conn in net.connections.items():
            if "w0_" + "_".join(key) in cases.gold("pool_" + name).files:
                assert np.array_equal(_bits(conn.w.detach().numpy()), _bits(cases.gold("pool_" + name)["w0_" + "_".join(key)])), "constructor draw"
        snaps = PC.run_case(net, name, Monitor)
    finally:
        torch.set_num_threads(n)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps)


@pytest.mark.parametrize("name", ["b", "e", "h", "m2"])
def test_two_halves_equal_one_whole_run(name):
    from bindsnet_amd.network.monitors import Monitor
    check_snapshots(name, PC.run_case(PC.build(_ns(), name), name, Monitor, split=True))


def test_compute_by_hand():
    import torch.nn.functional as F
    ns = _ns()
    c = PC.POOL["b"]
    net = PC.build(ns, "b")
    conn = PC.pool_of(net)
    assert tuple(conn.firing_rates.shape) == (c["B"], *c["shape"]) and conn.firing_rates.dtype == torch.float32
    x = torch.from_numpy(PC.inputs("b", 0))
    fr = torch.zeros(c["B"], *c["shape"])
    for t in range(4):
        out = conn.compute(x[t])
        fr = fr - c["decay"] * fr
        fr = fr + x[t].float()
        _, idx = F.max_pool2d(fr, c["k"], c["s"], c["p"], c["d"], return_indices=True)
        want = x[t].flatten(2).gather(2, idx.flatten(2)).view_as(idx).float()
        assert out.shape == (c["B"], *PC.pooled_shape(c)) and torch.equal(out, want)
        assert np.array_equal(_bits(conn.firing_rates.numpy()), _bits(fr.numpy()))
        taps = PC.window_taps(c)                                  # ... and the first maximum of the enumerated windows
        assert np.array_equal(PC.window_stats(fr.numpy(), taps)[0].reshape(-1), idx.numpy().reshape(-1))
    conn.reset_state_variables()
    assert not conn.firing_rates.any() and tuple(conn.firing_rates.shape) == (c["B"], *c["shape"])
    conn.normalize()                                              # no weights -> nothing
    # mean field: a tensor of w's shape, the mean over the batch too
    s = torch.from_numpy(PC.inputs("m1", 0))[0]
    for w in (torch.tensor(-0.5), torch.arange(20.0) - 3.0):
        mf = ns.MeanFieldConnection(ns.Input(n=50), ns.LIFNodes(n=20), w=w)
        got = mf.compute(s)
        assert got.shape == w.shape and np.array_equal(_bits(got.numpy()), _bits((s.float().mean() * w).numpy()))
        assert np.array_equal(_bits(got.numpy()), _bits((np.float32(int(s.sum())) / np.float32(s.numel()) * w.numpy()).astype(np.float32)))


@pytest.mark.parametrize("variant", sorted(PC.CTOR))
def test_meanfield_constructor_matches_the_reference(variant):
    g = cases.gold("pool_ctor")
    conn, probe = PC.ctor(_ns(), variant)
    assert isinstance(conn.w, torch.nn.Parameter) and not conn.w.requires_grad
    assert conn.w.shape == g[f"{variant}_w"].shape and np.array_equal(_bits(conn.w.detach().numpy()), _bits(g[f"{variant}_w"]))
    assert np.array_equal(_bits(probe), _bits(g[f"{variant}_gen"])), "the generator stands elsewhere behind the constructor"
    assert float(conn.update_rule.weight_decay) == float(g[f"{variant}_rule_decay"]) == 1.0      # weight_decay never reaches the rule


# what each call of pool_cases.CALLS must do HERE, given what the reference does (the fixture's record)
_SAME = ("pool_decay_none", "pool_b1", "pool_b1_c1", "pool_b2_c1", "pool_inner_one", "pool_target_shape", "pool_other_batch_without_reset",
         "mean_postpre", "mean_training_mode", "mean_weight_decay_training", "mean_recurrent_inhibition")
_DEVIATES = {"pool_training_mode": ("AttributeError", "ok"),            # deviation 1: nothing to learn, so it runs
             "pool_built_before_layers": ("RuntimeError", "ok"),        # deviation 2: zero rates of the right shape at first use
             "mean_norm": ("TypeError", "NotImplementedError")}         # refused before the run instead of failing behind it


def test_every_recorded_call_is_covered():
    g = cases.gold("pool_ctor")
    assert sorted(g["calls"].tolist()) == sorted(PC.CALLS) == sorted(_SAME + tuple(_DEVIATES))
    ref = dict(zip(g["calls"].tolist(), g["outcomes"].tolist()))
    assert ref["pool_decay_none"] == "TypeError" and ref["pool_b2_c1"] == ref["pool_inner_one"] == ref["pool_target_shape"] == "RuntimeError"
    assert ref["pool_b1"] == ref["pool_b1_c1"] == ref["mean_recurrent_inhibition"] == ref["mean_training_mode"] == "ok"
    assert ref["mean_postpre"] == "NotImplementedError"
    for call, (theirs, _) in _DEVIATES.items():
        assert ref[call] == theirs


@pytest.mark.parametrize("call", sorted(PC.CALLS))
def test_raises_as_the_reference_or_as_documented(call):
    g = cases.gold("pool_ctor")
    ref = dict(zip(g["calls"].tolist(), g["outcomes"].tolist()))
    want = _DEVIATES[call][1] if call in _DEVIATES else ref[call]
    assert PC.outcome(_ns(), call) == want


def _state(net):
    Y = net.layers["Y"]
    out = [t.clone() for t in (Y.v, Y.refrac_count, Y.x, Y.s)] + [torch.get_rng_state()]
    pool = PC.pool_of(net)
    return out + ([pool.firing_rates.clone()] if pool is not None else [])


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def test_refusals_come_before_the_run_changes_any_state():
    from bindsnet_amd.network.monitors import Monitor
    ns = _ns()
    x2 = lambda shape, B=2: {"X": torch.ones(3, B, *shape, dtype=torch.uint8)}       # noqa: E731
    mask = {("X", "Y"): torch.zeros(1, dtype=torch.bool)}
    table = [
        (lambda: PC._pool_net(ns, (2, 4, 4), 2, decay=None), x2((2, 4, 4)), {}, TypeError, "decay"),
        (lambda: PC._pool_net(ns, (1, 4, 4), 2), x2((1, 4, 4)), {}, RuntimeError, "squeeze"),
        (lambda: PC._pool_net(ns, (2, 1, 4), 2, target=(2, 1, 2)), x2((2, 1, 4)), {}, RuntimeError, "squeeze"),
        (lambda: PC._pool_net(ns, (2, 4, 4), 2, target=(8,)), x2((2, 4, 4)), {}, RuntimeError, "target's shape"),
        (lambda: PC._pool_net(ns, (2, 4, 4), 2), x2((2, 4, 4)), {"masks": mask}, NotImplementedError, "mask"),
        (lambda: PC._mean_net(ns, w=torch.tensor(0.5), norm=1.0), x2((6,)), {}, NotImplementedError, "TypeError"),
        (lambda: PC._mean_net(ns, w=torch.tensor(0.5)), x2((6,)), {"masks": mask}, NotImplementedError, "mask"),
        (lambda: PC._mean_net(ns, w=torch.ones(2, 3, 1)), x2((6,)), {}, NotImplementedError, "tail"),
    ]
    for make, x, kwargs, exc, match in table:
        net = make()
        before = _state(net)
        with pytest.raises(exc, match=match) as e:
            net.run(dict(x), time=3, **kwargs)
        assert type(e.value) is exc and _same(before, _state(net)), match
    # rates kept from another batch size, as in the reference: RuntimeError until reset_state_variables()
    net = PC._pool_net(ns, (2, 4, 4), 2)
    with pytest.raises(RuntimeError, match="reset_state_variables"):
        net.run(x2((2, 4, 4), B=3), time=3)
    net.reset_state_variables()
    net.run(x2((2, 4, 4), B=3), time=3)
    assert tuple(PC.pool_of(net).firing_rates.shape) == (3, 2, 4, 4)
    # monitors on either connection
    for make, x in ((lambda: PC._pool_net(ns, (2, 4, 4), 2), x2((2, 4, 4))), (lambda: PC._mean_net(ns, w=torch.tensor(0.5)), x2((6,)))):
        net = make()
        conn = net.connections[("X", "Y")]
        net.add_monitor(Monitor(conn, ["firing_rates" if PC.pool_of(net) is not None else "w"], time=3), name="m")
        before = _state(net)
        with pytest.raises(NotImplementedError, match="monitor"):
            net.run(dict(x), time=3)
        assert _same(before, _state(net))
    # at construction
    X, Y = ns.Input(n=6, traces=True), ns.LIFNodes(n=3, traces=True)
    from bindsnet_amd.learning import MSTDP, NoOp
    for rule in (ns.PostPre, MSTDP):
        with pytest.raises(NotImplementedError, match=r"^This learning rule is not supported for this Connection type\.$"):
            ns.MeanFieldConnection(X, Y, update_rule=rule, nu=1e-2)
    assert isinstance(ns.MeanFieldConnection(X, Y, update_rule=NoOp).update_rule, NoOp)
    with pytest.raises(NotImplementedError, match="Dales_rule"):
        ns.MeanFieldConnection(X, Y, Dales_rule=torch.ones(1))
    with pytest.raises(NotImplementedError, match="Dales_rule"):
        ns.pool[2](ns.Input(shape=(2, 4, 4)), ns.LIFNodes(shape=(2, 2, 2)), kernel_size=2, stride=2, decay=0.1, Dales_rule=torch.ones(1))
    with pytest.raises(NotImplementedError, match="float32"):
        ns.MeanFieldConnection(X, Y, w_dtype=torch.float64)
    net = PC._mean_net(ns, w=torch.tensor(0.5))
    net.connections[("X", "Y")].w = torch.nn.Parameter(torch.tensor(0.5, dtype=torch.float64), requires_grad=False)
    with pytest.raises(NotImplementedError, match="float32"):
        net.run(x2((6,)), time=3)
    from bindsnet_amd import parallel
    for net in (PC._pool_net(ns, (2, 4, 4), 2), PC._mean_net(ns, w=torch.tensor(0.5))):
        with pytest.raises(NotImplementedError, match="MaxPool2dConnection|MeanFieldConnection"):
            parallel._refuse(net, "sharded_run")


def test_meanfield_refuses_more_than_2_24_source_elements():
    ns = _ns()
    net = ns.Network(dt=1.0, batch_size=2)
    net.add_layer(ns.Input(n=(1 << 23) + 1), name="X")
    net.add_layer(ns.LIFNodes(n=3), name="Y")
    net.add_connection(ns.MeanFieldConnection(net.layers["X"], net.layers["Y"], w=torch.tensor(0.5)), source="X", target="Y")
    with pytest.raises(NotImplementedError, match=r"2\^24"):
        net.run({"X": torch.zeros(1, 2, (1 << 23) + 1, dtype=torch.uint8)}, time=1)


def test_entry_points_reject_bad_arguments_before_any_launch():
    """Argument checks of the two entry points return before anything is launched: no GPU needed."""
    import ctypes as C
    from bindsnet_amd import _lib
    L = _lib.lib()
    three = lambda *v: (C.c_int * 3)(*v)       # noqa: E731
    ok = (three(1, 6, 6), three(1, 2, 2), three(1, 2, 2), three(0, 0, 0), three(1, 1, 1))
    assert L.snn_prop_pool_f32(None, 1, 1, 1, 1, *ok, 0.1, 0, None) == -1
    assert L.snn_prop_pool_f32(1, 1, 1, 0, 1, *ok, 0.1, 0, None) == -1
    assert L.snn_prop_pool_f32(1, 1, 1, 1, 1, three(1, 6, 6), three(1, 2, 2), three(1, 2, 2), three(0, 2, 0), three(1, 1, 1), 0.1, 0, None) == -1   # pad > k / 2
    assert L.snn_prop_pool_f32(1, 1, 1, 1, 1, three(1, 2, 2), three(1, 3, 3), three(1, 1, 1), three(0, 0, 0), three(1, 1, 1), 0.1, 0, None) == -1   # empty output
    assert L.snn_prop_pool_f32(1, 1, 1, 1, 1, three(1, 6, 6), three(1, 2, 0), three(1, 2, 2), three(0, 0, 0), three(1, 1, 1), 0.1, 0, None) == -1
    assert L.snn_prop_pool_f32(1, 1, 1, 1 << 20, 1 << 20, *ok, 0.1, 0, None) == -2
    assert L.snn_prop_meanfield_f32(None, 1, 1, 1, 1, 1, 1, 0, None) == -1
    assert L.snn_prop_meanfield_f32(1, 2, 1, 1, 1, 4, 3, 0, None) == -1                 # w_numel does not divide B * n_tgt
    assert L.snn_prop_meanfield_f32(1, 1, 1, 1, 1, 4, 3, 3, None) == -1                 # no such accumulate mode
    assert L.snn_prop_meanfield_f32(1, 1, 1, 1, 2, (1 << 23) + 1, 3, 0, None) == -2
    hdr = open(cases.os.path.join(cases.os.path.dirname(cases.GOLD), "..", "include", "snnhip.h")).read()
    assert f"#define SNN_POOL_STAGE {_lib.POOL_STAGE}\n" in hdr and f"#define SNN_MEANFIELD_STORE {_lib.MEANFIELD_STORE}\n" in hdr
