"""AvgPool2dConnection on the MI355X: ops.prop_avgpool (snn_prop_avgpool2d_f32, csrc/snn_avgpool.hip) against F.avg_pool2d on the
CPU, bit for bit, through both of its bodies; a pooling graph and a converted CNN with BatchNorm and average pooling through
Network.run, device against host path, bit for bit; the device-side refusals."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import avgpool_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 20


def _parts():
    from bindsnet_amd.conversion import SubtractiveResetIFNodes
    from bindsnet_amd.network import Network, nodes, topology
    from bindsnet_amd.network.monitors import Monitor
    return dict(Input=nodes.Input, SIF=SubtractiveResetIFNodes), topology, Network, Monitor


def _device(s, geometry_kwargs, body=0, prev=None):
    """ops.prop_avgpool over s on the device, in front of and behind guard elements; body: snn_set_avgpool_body."""
    from bindsnet_amd import _lib, ops
    arrays, pooled = ops.avgpool_geometry(s.shape[2:], geometry_kwargs["kernel_size"], geometry_kwargs["stride"], geometry_kwargs["padding"],
                                          geometry_kwargs["ceil_mode"])
    n = s.shape[0] * s.shape[1] * pooled[0] * pooled[1]
    flat = torch.full((n + 128,), -5.0, device=DEV)
    out = flat[64:64 + n].view(s.shape[0], s.shape[1], *pooled)
    if prev is not None:
        out.copy_(prev)
    _lib.lib().snn_set_avgpool_body(body)
    try:
        ops.prop_avgpool(s.to(DEV), out, accumulate=prev is not None, **geometry_kwargs)
        torch.cuda.synchronize()
    finally:
        _lib.lib().snn_set_avgpool_body(0)
    assert bool((flat[:64] == -5.0).all()) and bool((flat[64 + n:] == -5.0).all()), "a write outside the output"
    return out.cpu()


# planes 7x5, 6x6, 9x11 at B = 3, C = 4: kernel 2x3 with stride 1x2; 3x3, stride 2, pad 1 under both count_include_pad values; ceil_mode
# with a window running off the end (kernel 2, stride 2 on the odd sizes; 3x3, stride 3, pad 1); divisor_override
SWEEP = [g for g in AC.GEOMETRIES if (g[1], g[2], g[3], g[4]) in {((2, 3), (1, 2), 0, False), ((3, 3), (2, 2), 1, False), ((2, 2), (2, 2), 0, True),
                                                                  ((3, 3), (3, 3), 1, True), ((6, 5), (1, 2), 1, True)}]


def test_device_op_equals_torch_on_the_sweep():
    """Fewer than AVGPOOL_COOP_TAPS taps: the per-thread body; every case again through the per-wave body; bool and uint8 spikes."""
    from bindsnet_amd import _lib
    assert len(SWEEP) == 30 and all(g[1][0] * g[1][1] < _lib.AVGPOOL_COOP_TAPS for g in SWEEP)
    for g in SWEEP:
        for divisor in AC.DIVISORS:
            want = AC.reference(g, divisor)
            for body, dtype in ((0, torch.uint8), (0, torch.bool), (2, torch.uint8)):
                assert AC.same_bits(_device(AC.spikes(g[0]).to(dtype), AC.pool_kwargs(g, divisor), body=body), want), (g, divisor, body, dtype)


def test_whole_plane_window_takes_the_cooperative_body():
    """Global pooling: 9 * 11 = 99 taps and 32 * 32 = 1024 taps per output, AVGPOOL_COOP_TAPS and more -- the per-wave body under the rule
    (body 0); the per-thread body must give the same bits."""
    from bindsnet_amd import _lib
    for plane in ((9, 11), (32, 32)):
        assert plane[0] * plane[1] >= _lib.AVGPOOL_COOP_TAPS
        s = AC.spikes(plane)
        kw = dict(kernel_size=plane, stride=plane, padding=0, ceil_mode=False, count_include_pad=True, divisor_override=None)
        want = F.avg_pool2d(s.float(), plane)
        assert 0 < float(want.min()) and float(want.max()) < 1
        for body in (0, 1):
            assert AC.same_bits(_device(s, kw, body=body), want), (plane, body)
    # a large window that is not the whole plane: rows of the window are not adjacent in memory, windows overlap, padding clips them
    s = AC.spikes((32, 32))
    kw = dict(kernel_size=(9, 8), stride=(5, 7), padding=(4, 3), ceil_mode=True, count_include_pad=False, divisor_override=None)
    assert AC.same_bits(_device(s, kw), F.avg_pool2d(s.float(), **kw))


def test_more_outputs_than_one_pass_of_the_grid():
    """B = 2, C = 3, plane 257 x 259, kernel 2, stride 1: 2 * 3 * 256 * 258 = 396288 outputs.  One pass of the per-thread body is
    AVGPOOL_MAX_GRID * AVGPOOL_THREADS = 262144 outputs, one pass of the per-wave body AVGPOOL_MAX_GRID * AVGPOOL_THREADS / 64 = 4096: both
    bodies must stride on."""
    from bindsnet_amd import _lib
    s = AC.spikes((257, 259), b=2, c=3)
    kw = dict(kernel_size=(2, 2), stride=(1, 1), padding=0, ceil_mode=False, count_include_pad=True, divisor_override=None)
    want = F.avg_pool2d(s.float(), 2, 1)
    assert want.numel() == 396288 > _lib.AVGPOOL_MAX_GRID * _lib.AVGPOOL_THREADS
    for body in (0, 2):
        assert AC.same_bits(_device(s, kw, body=body), want), body


def test_accumulate_adds_onto_a_non_zero_out():
    gen = torch.Generator().manual_seed(6)
    for g in SWEEP[::5]:
        want = AC.reference(g)
        prev = torch.rand(want.shape, generator=gen) * 3 - 1
        for body in (0, 2):
            assert AC.same_bits(_device(AC.spikes(g[0]), AC.pool_kwargs(g), body=body, prev=prev), prev + want), (g, body)


def test_compute_on_device_tensors():
    kinds, topology, _, _ = _parts()
    g = ((7, 5), (2, 3), (1, 2), 1, True, False)
    conn = topology.AvgPool2dConnection(kinds["Input"](shape=(AC.C, 7, 5)), kinds["SIF"](shape=tuple(AC.reference(g).shape[1:])), **AC.pool_kwargs(g))
    out = conn.compute(AC.spikes((7, 5), torch.bool).to(DEV))
    assert out.is_cuda and AC.same_bits(out, AC.reference(g))


# ---- Network.run: device against host path ------------------------------------------------------------------------------------------

def _run_graph(b, device, halves=False):
    kinds, topology, Network, Monitor = _parts()
    net = AC.pool_graph(kinds, topology, Network, b)
    x = AC.model_input(T, b, seed=40)
    if device:
        net.to(DEV)
        x = x.to(DEV)
    names = ("A", "P", "Y")
    for n in names:
        net.add_monitor(Monitor(net.layers[n], ["s"], time=T), name=f"{n}_s")
    for piece in ((x[:T // 2], x[T // 2:]) if halves else (x,)):
        net.run({"X": piece.clone()}, time=piece.shape[0])
    out = {f"{n}_raster": net.monitors[f"{n}_s"].get("s").cpu() != 0 for n in names}
    out.update({f"{n}_v": net.layers[n].v.detach().cpu() for n in names})
    out["Y_summed"] = net.layers["Y"].summed.detach().cpu()
    return net, out


@pytest.mark.parametrize("b", [1, 3])
def test_pooling_graph_device_equals_host(b):
    _, host = _run_graph(b, device=False)
    pooled = host["P_raster"]
    assert 0 < int(pooled.sum()) < pooled.numel(), "the pooled layer's raster must be neither empty nor all ones"
    net, dev = _run_graph(b, device=True)
    assert net.last_plan == "generic"
    for k in host:
        if k.endswith("_raster"):
            assert torch.equal(dev[k].reshape(host[k].shape), host[k]), k
        else:
            assert AC.same_bits(dev[k].reshape(host[k].shape), host[k]), k
    _, halves = _run_graph(b, device=True, halves=True)
    for k in dev:
        assert torch.equal(halves[k], dev[k]) if k.endswith("_raster") else AC.same_bits(halves[k], dev[k]), f"two half runs: {k}"


@pytest.mark.parametrize("b", [1, 3])
def test_converted_batchnorm_model_device_equals_host(b):
    """BatchNorm scales are powers of two and every parameter lies on a dyadic grid (avgpool_cases.model), so every partial sum is exact
    and the device's summation orders cannot show: every raster, v and summed bit for bit."""
    from bindsnet_amd.conversion import ann_to_snn
    _, _, _, Monitor = _parts()
    x = AC.model_input(T, b)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        host = AC.run_converted(ann_to_snn(AC.model(), AC.INPUT), x, Monitor)
        net = ann_to_snn(AC.model(), AC.INPUT).to(DEV)
    dev = AC.run_converted(net, x.to(DEV), Monitor)
    assert net.last_plan == "generic"
    for name in host[0]:
        assert 0 < int(host[0][name].sum()) < host[0][name].numel(), name
        assert torch.equal(dev[0][name], host[0][name]) and AC.same_bits(dev[1][name], host[1][name]), name
    assert AC.same_bits(dev[2], host[2])


# ---- refusals on the device, each before any state changes ---------------------------------------------------------------------------

def _net(target=None, conn_of=None):
    kinds, topology, Network, _ = _parts()
    net = Network(dt=1.0, batch_size=2)
    X = kinds["Input"](shape=(2, 6, 6))
    P = target if target is not None else kinds["SIF"](shape=(2, 3, 3), reset=0, thresh=1, refrac=0)
    net.add_layer(X, name="X")
    net.add_layer(P, name="P")
    net.add_connection(conn_of(X, P) if conn_of else topology.AvgPool2dConnection(X, P, kernel_size=2), "X", "P")
    return net.to(DEV)


def _refused(net, exc, match, **run):
    state = lambda: [getattr(l, k).detach().clone() for l in net.layers.values() for k in ("v", "s") if isinstance(getattr(l, k, None), torch.Tensor)]     # noqa: E731
    before, rng = state(), torch.get_rng_state()
    with pytest.raises(exc, match=match):
        net.run(**run)
    assert all(torch.equal(a, b) for a, b in zip(before, state())) and torch.equal(rng, torch.get_rng_state()), "a refused run changed state"


def test_refusals_on_the_device():
    from bindsnet_amd.conversion import PassThroughNodes
    kinds, topology, _, Monitor = _parts()
    name = "AvgPool2dConnection"
    x = (torch.rand(3, 2, 2, 6, 6) < 0.5).byte().to(DEV)
    run = dict(inputs={"X": x}, time=3)
    good = _net()
    good.layers["P"].v.fill_(0.25)
    _refused(good, NotImplementedError, f"{name} out of the Input layer 'X' takes no real-valued", inputs={"X": torch.rand(3, 2, 2, 6, 6, device=DEV)}, time=3)
    _refused(good, NotImplementedError, f"mask on an {name}", masks={("X", "P"): torch.ones(72, 18)}, **run)
    good.add_monitor(Monitor(good.connections[("X", "P")], ["kernel_size"], time=3), name="c")
    _refused(good, NotImplementedError, f"monitor on an {name}", **run)
    del good.monitors["c"]
    _refused(_net(target=kinds["SIF"](shape=(2, 3, 2), reset=0, thresh=1, refrac=0)), RuntimeError, f"{name}: the target's shape", **run)
    _refused(_net(target=PassThroughNodes(shape=(2, 3, 3))), NotImplementedError, f"{name} into", **run)
    reason = good.connections[("X", "P")]._multi_device_refusal("exact_run", ("X", "P"))
    assert isinstance(reason, NotImplementedError) and name in str(reason)
    good.run(**run)                                                                        # ... and the graph itself runs
    assert good.last_plan == "generic" and not torch.equal(good.layers["P"].v, torch.full_like(good.layers["P"].v, 0.25))
