"""AvgPool2dConnection and fold_batchnorm on the HOST (no GPU): the class and its facts, `compute` against F.avg_pool2d on the 576
geometries of tests/avgpool_cases.py (and with divisor_override = 3), every refusal before a run changes state, BatchNorm folding
against a numpy float64 restatement, and what ann_to_snn builds from a CNN with BatchNorm and average pooling -- its run against a
plain-torch step loop, bit for bit."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import avgpool_cases as AC

T = 20


def _parts():
    from bindsnet_amd.conversion import SubtractiveResetIFNodes
    from bindsnet_amd.network import Network, nodes, topology
    from bindsnet_amd.network.monitors import Monitor
    return dict(Input=nodes.Input, SIF=SubtractiveResetIFNodes, IF=nodes.IFNodes), topology, Network, Monitor


def _pair(plane, geometry_kwargs, target=None, c=AC.C, **extra):
    """An AvgPool2dConnection over a (c, *plane) Input with a target of the pooled shape."""
    kinds, topology, _, _ = _parts()
    pooled = F.avg_pool2d(torch.empty(1, c, *plane, device="meta"), **{k: v for k, v in geometry_kwargs.items()
                                                                        if k not in ("count_include_pad", "divisor_override")}).shape[1:]
    src = kinds["Input"](shape=(c, *plane))
    tgt = target if target is not None else kinds["IF"](shape=tuple(pooled))
    return topology.AvgPool2dConnection(src, tgt, **geometry_kwargs, **extra)


def test_the_class_resolves_from_both_names():
    import bindsnet.network.topology as alias
    from bindsnet_amd import _lib
    from bindsnet_amd.network import topology
    assert alias.AvgPool2dConnection is topology.AvgPool2dConnection
    cls = topology.AvgPool2dConnection
    assert cls._kind == _lib.CONN_AVGPOOL == 10
    assert cls._rules == {"NoOp"} and cls._takes_mask is False and cls._multi_device is False and cls._takes_real is False
    conn = _pair((6, 6), dict(kernel_size=2))
    assert conn.stride == (2, 2) and conn.padding == (0, 0) and conn.divisor_override is None        # stride None: the kernel's, as torch
    assert not hasattr(conn, "w") and not list(conn.buffers(recurse=False)), "no weights, no state"
    assert {n for n, _ in conn.named_parameters(recurse=False)} == {"wmin", "wmax"}                   # (what every connection carries)
    assert type(conn.update_rule).__name__ == "NoOp"
    from bindsnet_amd.learning import PostPre
    with pytest.raises(NotImplementedError):
        _pair((6, 6), dict(kernel_size=2), update_rule=PostPre, nu=1e-2)
    with pytest.raises(NotImplementedError, match="AvgPool2dConnection"):
        _pair((6, 6), dict(kernel_size=2), Dales_rule=torch.ones(1))
    with pytest.raises(ValueError, match="divisor_override"):
        _pair((6, 6), dict(kernel_size=2), divisor_override=0)


def test_descriptor_fields_and_geometry_mirror():
    """The ctypes mirror carries the avgp_* fields, and ops.avgpool_geometry computes ATen's output sizes on every geometry."""
    from bindsnet_amd import _lib, ops
    d = _lib.ConnDesc()
    conn = _pair((7, 5), dict(kernel_size=(2, 3), stride=(1, 2), padding=1, ceil_mode=True, count_include_pad=False, divisor_override=3))
    assert conn._describe(d, 2, torch.device("cpu"), None) == []
    assert (d.kind, d.w, d.avgp_c, list(d.avgp_in), list(d.avgp_k), list(d.avgp_stride), list(d.avgp_pad)) == \
        (10, None, AC.C, [7, 5], [2, 3], [1, 2], [1, 1])
    assert (d.avgp_ceil, d.avgp_include_pad, d.avgp_divisor) == (1, 0, 3)
    for g in AC.GEOMETRIES:
        plane, k, stride, pad, ceil_mode, _ = g
        assert ops.avgpool_geometry(plane, k, stride, pad, ceil_mode)[1] == tuple(AC.reference(g).shape[2:]), g


def test_host_compute_equals_torch_on_every_geometry():
    assert len(AC.GEOMETRIES) * len(AC.DIVISORS) == 576
    fractions = 0
    for g in AC.GEOMETRIES:
        for divisor in AC.DIVISORS:
            want = AC.reference(g, divisor)
            conn = _pair(g[0], AC.pool_kwargs(g, divisor))
            for dtype in (torch.uint8, torch.bool):
                got = conn.compute(AC.spikes(g[0]).to(dtype))
                assert AC.same_bits(got, want), (g, divisor, dtype)
            fractions += int(((want > 0) & (want < 1)).sum())
    assert fractions > 10000, "the geometries must produce real fractions"


def _net(conn_of=None, target=None, plane=(6, 6)):
    kinds, topology, Network, _ = _parts()
    net = Network(dt=1.0, batch_size=2)
    X = kinds["Input"](shape=(2, *plane))
    P = target if target is not None else kinds["SIF"](shape=(2, plane[0] // 2, plane[1] // 2), reset=0, thresh=1, refrac=0)
    net.add_layer(X, name="X")
    net.add_layer(P, name="P")
    net.add_connection(conn_of(X, P) if conn_of else topology.AvgPool2dConnection(X, P, kernel_size=2), "X", "P")
    return net


def _state(net):
    return [getattr(l, k).detach().clone() for l in net.layers.values() for k in ("v", "s", "summed") if isinstance(getattr(l, k, None), torch.Tensor)]


def _refused(net, exc, match, **run):
    before, rng = _state(net), torch.get_rng_state()
    with pytest.raises(exc, match=match):
        net.run(**run)
    assert all(torch.equal(a, b) for a, b in zip(before, _state(net))) and torch.equal(rng, torch.get_rng_state()), "a refused run changed state"


def test_refusals_come_before_any_state_changes():
    from bindsnet_amd.conversion import PassThroughNodes
    from bindsnet_amd.network import topology
    from bindsnet_amd.network._preflight import RunRequest
    from bindsnet_amd.network.monitors import Monitor
    x = (torch.rand(3, 2, 2, 6, 6) < 0.5).byte()
    run = dict(inputs={"X": x}, time=3)
    name = "AvgPool2dConnection"
    good = _net()
    good.layers["P"].v.fill_(0.25)                                                         # (state a refused run must leave alone)
    _refused(good, NotImplementedError, f"mask on an {name}", masks={("X", "P"): torch.ones(72, 18)}, **run)
    good.add_monitor(Monitor(good.connections[("X", "P")], ["kernel_size"], time=3), name="c")
    _refused(good, NotImplementedError, f"monitor on an {name}", **run)
    del good.monitors["c"]
    kinds = _parts()[0]
    _refused(_net(target=kinds["SIF"](shape=(2, 3, 2), reset=0, thresh=1, refrac=0)), RuntimeError, f"{name}: the target's shape must be \\(2, 3, 3\\)", **run)
    _refused(_net(target=PassThroughNodes(shape=(2, 3, 3))), NotImplementedError, f"{name} into a PassThroughNodes", **run)
    _refused(_net(conn_of=lambda a, b: topology.AvgPool2dConnection(a, b, kernel_size=2, padding=2)), RuntimeError, name, **run)   # torch: pad beyond half the kernel
    # a real-valued Input: asked as the device run asks (the host path takes floats as torch does); the multi-device modes
    req = RunRequest.of(good, {"X": torch.rand(3, 2, 2, 6, 6)}, 3, on_device=True)
    reasons = [e for e in good._preflight(req) if e is not None]
    assert any(isinstance(e, NotImplementedError) and name in str(e) and "real-valued" in str(e) for e in reasons), reasons
    reason = good.connections[("X", "P")]._multi_device_refusal("column_shard", ("X", "P"))
    assert isinstance(reason, NotImplementedError) and name in str(reason)
    assert list(good._preflight(RunRequest.of(good, run["inputs"], 3))) == []
    good.run(**run)                                                                        # ... and the graph itself runs
    assert good.last_plan == "host-torch" and not torch.equal(good.layers["P"].v, torch.full_like(good.layers["P"].v, 0.25))


# ---- fold_batchnorm ----------------------------------------------------------------------------------------------------------------

def _bn_models():
    torch.manual_seed(21)
    cnn = AC.model(dyadic=False)
    mlp = nn.Sequential(nn.Linear(7, 6, bias=False), nn.BatchNorm1d(6, affine=False), nn.ReLU(), nn.Linear(6, 4), nn.BatchNorm1d(4, eps=1e-3)).eval()
    with torch.no_grad():
        for m in mlp:
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                if m.affine:
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.normal_(0, 0.3)
    return cnn, mlp


def test_fold_batchnorm_equals_the_float64_rule_bit_for_bit():
    import bindsnet.conversion
    from bindsnet_amd.conversion import conversion
    assert bindsnet.conversion.fold_batchnorm is conversion.fold_batchnorm and "fold_batchnorm" not in bindsnet.conversion.__all__
    for ann in _bn_models():
        kept = [(type(m), None if not hasattr(m, "weight") or m.weight is None else m.weight.detach().numpy().copy(),
                 None if getattr(m, "bias", None) is None else m.bias.detach().numpy().copy()) for m in ann]
        stats = [(m.running_mean.numpy().copy(), m.running_var.numpy().copy(), m.eps) if isinstance(m, nn.modules.batchnorm._BatchNorm) else None for m in ann]
        names = [n for n, _ in ann.named_children()]
        assert conversion.fold_batchnorm(ann) is ann
        assert [n for n, _ in ann.named_children()] == names, "no child moves"
        folded = 0
        for i, m in enumerate(ann):
            if stats[i] is None:
                continue
            assert isinstance(m, nn.Identity) and isinstance(ann[i - 1], (nn.Conv2d, nn.Linear))
            mean, var, eps = stats[i]
            w, b = AC.np_fold(kept[i - 1][1], kept[i - 1][2], kept[i][1], kept[i][2], mean, var, eps)
            assert ann[i - 1].bias is not None, "a layer without bias gains one"
            assert AC.same_bits(ann[i - 1].weight, torch.from_numpy(w)) and AC.same_bits(ann[i - 1].bias, torch.from_numpy(b)), i
            assert not np.array_equal(w, kept[i - 1][1])
            folded += 1
        assert folded == 2
        assert conversion.fold_batchnorm(ann) is ann                                       # nothing left to fold: nothing changes
    plain = nn.Sequential(nn.Conv2d(1, 2, 3), nn.ReLU(), nn.Flatten(), nn.Linear(8, 3))
    before = [p.detach().clone() for p in plain.parameters()]
    conversion.fold_batchnorm(plain)
    assert all(AC.same_bits(a, b) for a, b in zip(before, plain.parameters())) and [type(m) for m in plain] == [nn.Conv2d, nn.ReLU, nn.Flatten, nn.Linear]


def test_fold_batchnorm_refuses_what_it_cannot_fold():
    from bindsnet_amd.conversion.conversion import fold_batchnorm
    with pytest.raises(ValueError, match="BatchNorm2d child '1'.*running statistics"):
        fold_batchnorm(nn.Sequential(nn.Conv2d(1, 2, 3), nn.BatchNorm2d(2, track_running_stats=False)))
    with pytest.raises(NotImplementedError, match="BatchNorm2d child '2'.*not directly behind a Conv2d"):
        fold_batchnorm(nn.Sequential(nn.Conv2d(1, 2, 3), nn.ReLU(), nn.BatchNorm2d(2)))
    with pytest.raises(NotImplementedError, match="BatchNorm2d child '0'"):
        fold_batchnorm(nn.Sequential(nn.BatchNorm2d(1), nn.Conv2d(1, 2, 3)))              # (forward-folding: out of scope)
    with pytest.raises(NotImplementedError, match="BatchNorm1d child '1'.*not directly behind a Linear"):
        fold_batchnorm(nn.Sequential(nn.Conv2d(1, 2, 3), nn.BatchNorm1d(2)))
    ann = nn.Sequential(nn.Conv2d(1, 2, 3), nn.ReLU(), nn.BatchNorm2d(2))
    before = [p.detach().clone() for p in ann.parameters()]
    with pytest.raises(NotImplementedError):
        fold_batchnorm(ann)
    assert all(torch.equal(a, b) for a, b in zip(before, ann.parameters()))


def test_folded_model_stays_within_four_times_the_float32_error():
    """E0: the float32 model's distance from its float64 self on a fixed batch.  Folding adds one rounding per weight and per bias, so the
    folded float32 model must lie within 4 * E0.  Measured: CNN E0 = 6.53e-08, folded 5.48e-08; MLP E0 = 5.16e-08, folded 6.55e-08."""
    from copy import deepcopy
    from bindsnet_amd.conversion.conversion import fold_batchnorm
    gen = torch.Generator().manual_seed(33)
    for ann, x in zip(_bn_models(), (torch.rand(16, *AC.INPUT, generator=gen), torch.rand(16, 7, generator=gen))):
        with torch.no_grad():
            exact = deepcopy(ann).double()(x.double())
            e0 = float((ann(x).double() - exact).abs().max())
            e1 = float((fold_batchnorm(deepcopy(ann))(x).double() - exact).abs().max())
        print(f"{type(ann[0]).__name__} model: E0 = {e0:.3g}, folded = {e1:.3g}")
        assert e0 > 0 and e1 <= 4 * e0, (e0, e1)


# ---- ann_to_snn ---------------------------------------------------------------------------------------------------------------------

def _converted(ann, **kwargs):
    from bindsnet_amd.conversion import ann_to_snn
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return ann_to_snn(ann, AC.INPUT, **kwargs)


def test_ann_to_snn_builds_the_pooling_and_folds_the_batchnorm():
    ann = AC.model()
    kept = [p.detach().clone() for p in ann.parameters()]
    net = _converted(ann)
    assert [(k, type(l).__name__, [int(x) for x in l.shape]) for k, l in net.layers.items()] == AC.MODEL_LAYERS
    assert [(list(k), type(c).__name__) for k, c in net.connections.items()] == AC.MODEL_CONNECTIONS
    assert all(torch.equal(a, b) for a, b in zip(kept, ann.parameters())) and isinstance(ann[1], nn.BatchNorm2d), "the caller's model is left alone"
    last = net.layers["10"]
    assert last.sum_input and all(not l.sum_input for n, l in net.layers.items() if n not in ("Input", "10"))
    pool, glob = net.connections[("3", "4")], net.connections[("7", "8")]
    assert (pool.kernel_size, pool.stride, pool.padding, pool.ceil_mode, pool.count_include_pad, pool.divisor_override) == ((2, 2), (2, 2), (0, 0), False, True, None)
    assert (glob.kernel_size, glob.stride) == ((4, 4), (4, 4))
    w, b = AC.np_fold(ann[0].weight.detach(), ann[0].bias.detach(), ann[1].weight.detach(), ann[1].bias.detach(), ann[1].running_mean, ann[1].running_var, ann[1].eps)
    assert AC.same_bits(net.connections[("0", "1")].w, torch.from_numpy(w)) and AC.same_bits(net.connections[("0", "1")].b, torch.from_numpy(b))
    # the module's own parameters reach the connection; a None entry of an adaptive size keeps that size
    odd = nn.Sequential(nn.AvgPool2d((2, 3), stride=(1, 2), padding=1, ceil_mode=True, count_include_pad=False, divisor_override=5), nn.AdaptiveAvgPool2d((None, 1)),
                        nn.Flatten(), nn.Linear(16, 3))
    net2 = _converted(odd)
    c = net2.connections[("0", "1")]
    assert (c.kernel_size, c.stride, c.padding, c.ceil_mode, c.count_include_pad, c.divisor_override) == ((2, 3), (1, 2), (1, 1), True, False, 5)
    assert tuple(net2.layers["1"].shape) == tuple(F.avg_pool2d(torch.empty(1, *AC.INPUT), (2, 3), (1, 2), 1, True).shape[1:]) == (2, 9, 5)
    assert net2.connections[("1", "2")].kernel_size == (1, 5) and tuple(net2.layers["2"].shape) == (2, 9, 1)
    with pytest.raises(NotImplementedError, match=r"\(8, 8\).*\(3, 3\)"):
        _converted(nn.Sequential(nn.AdaptiveAvgPool2d(3), nn.Flatten(), nn.Linear(18, 3)))
    with pytest.raises(NotImplementedError, match="BatchNorm2d child '1'"):
        _converted(nn.Sequential(nn.ReLU(), nn.BatchNorm2d(2), nn.Flatten(), nn.Linear(128, 3)))


@pytest.mark.parametrize("b", [1, 3])
def test_converted_run_equals_a_plain_torch_step_loop(b):
    _, _, _, Monitor = _parts()
    ann = AC.model()
    x = AC.model_input(T, b)
    want_r, want_v, want_sum = AC.step_loop(ann, x)
    rasters, v, summed = AC.run_converted(_converted(ann), x, Monitor)
    for name in want_r:
        assert torch.equal(rasters[name].reshape(want_r[name].shape), want_r[name]), name
        assert AC.same_bits(v[name].reshape(want_v[name].shape), want_v[name]), name
        assert 0 < int(want_r[name].sum()) < want_r[name].numel(), f"layer {name}: a raster that is all zeros or all ones checks nothing"
    assert AC.same_bits(summed.reshape(want_sum.shape), want_sum)
    halves = AC.run_converted(_converted(ann), x, Monitor, halves=True)
    assert all(torch.equal(halves[0][n], rasters[n]) and AC.same_bits(halves[1][n], v[n]) for n in rasters) and AC.same_bits(halves[2], summed)


def test_a_model_without_batchnorm_or_average_pooling_converts_as_before():
    """The five module types of the reference: the same layers, keys and weights as converting by hand what ann_to_snn did before."""
    torch.manual_seed(4)
    ann = nn.Sequential(nn.Conv2d(2, 3, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2), nn.Flatten(), nn.Linear(48, 4))
    data = torch.rand(8, *AC.INPUT)
    from copy import deepcopy
    from bindsnet_amd.conversion import data_based_normalization
    for kwargs in ({}, {"data": data}):
        net = _converted(ann, **kwargs)
        ref = data_based_normalization(deepcopy(ann), data) if kwargs else ann
        assert [(k, type(l).__name__) for k, l in net.layers.items()] == [("Input", "Input"), ("1", "SubtractiveResetIFNodes"), ("3", "PassThroughNodes"),
                                                                         ("5", "SubtractiveResetIFNodes")]
        assert [type(c).__name__ for c in net.connections.values()] == ["Conv2dConnection", "MaxPool2dConnection", "Connection"]
        assert AC.same_bits(net.connections[("0", "1")].w, ref[0].weight) and AC.same_bits(net.connections[("0", "1")].b, ref[0].bias)
        assert AC.same_bits(net.connections[("4", "5")].w, ref[4].weight.t()) and AC.same_bits(net.connections[("4", "5")].b, ref[4].bias)
