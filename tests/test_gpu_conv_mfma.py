"""snn_prop_conv2d_mfma_f32 on the device.  Operator: ops.prop_conv2d_mfma bit for bit (uint32 views) against the numpy restatement of
the stated order and against ops.prop_conv2d, at the smallest shapes at which each mechanism can break (tests/conv_mfma_cases.py).
Network: twins that differ only in prop_auto on a 20 -> 24 convolution give the same rasters and potentials, whole or in two halves."""
import numpy as np
import pytest
import torch

from conv_mfma_cases import SHAPES, case, stated_order

pytestmark = pytest.mark.gpu
DEV, T, B = "cuda", 20, 3


def _run(name, W, bias, s, oshape, shape, prev=None, **kw):
    from bindsnet_amd import ops
    out = torch.full(oshape, 7.5, device=DEV) if prev is None else torch.from_numpy(prev).to(DEV)
    getattr(ops, name)(torch.from_numpy(W).to(DEV), torch.from_numpy(s).to(DEV), out, bias=None if bias is None else torch.from_numpy(bias).to(DEV),
                       stride=shape[3], pad=shape[4], accumulate=prev is not None, **kw)
    return out.cpu().numpy().view(np.uint32)


def _want(W, s, bias, shape, prev=None):
    return stated_order(W, s, bias, shape[3], shape[4], prev).view(np.uint32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "x".join(map(str, sh)))
def test_operator_equals_the_stated_order_and_prop_conv2d(shape):
    W, bias, s, oshape = case(shape)
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    got = _run("prop_conv2d_mfma", W, bias, s, oshape, shape, counters=cnt)
    assert np.array_equal(got, _want(W, s, bias, shape)) and np.array_equal(got, _run("prop_conv2d", W, bias, s, oshape, shape))
    assert cnt[0].item() > 0 and cnt[1].item() == 0


def test_operator_variants_on_one_shape():
    shape = SHAPES[1]
    W, bias, s, oshape = case(shape, seed=3)
    prev = np.random.RandomState(5).randn(*oshape).astype(np.float32)
    assert np.array_equal(_run("prop_conv2d_mfma", W, None, s, oshape, shape), _want(W, s, None, shape))
    assert np.array_equal(_run("prop_conv2d_mfma", W, bias, s, oshape, shape, prev=prev), _want(W, s, bias, shape, prev))
    silent = _run("prop_conv2d_mfma", W, bias, np.zeros_like(s), oshape, shape)
    assert np.array_equal(silent, np.broadcast_to(bias[None, :, None, None], oshape).view(np.uint32))
    # bytes from {0, 1, 2, 3}: every workgroup meets one above 1 and takes the scalar body
    W, bias, s4, _ = case(shape, seed=4, levels=4, density=0.6)
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    got = _run("prop_conv2d_mfma", W, bias, s4, oshape, shape, counters=cnt)
    assert s4.max() == 3 and np.array_equal(got, _run("prop_conv2d", W, bias, s4, oshape, shape)) and np.array_equal(got, _want(W, s4, bias, shape))
    assert cnt.tolist()[0] == 0 and cnt.tolist()[1] > 0


def _net_run(ask, pieces):
    """Input (3, 8, 8) -> Conv 3 -> 20 -> IF -> Conv 20 -> 24 (prop_auto=ask) -> IF over T steps in `pieces` calls: rasters, v, stats."""
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.monitors import Monitor
    from bindsnet_amd.network.nodes import IFNodes, Input
    from bindsnet_amd.network.topology import Conv2dConnection as Conv
    g = torch.Generator().manual_seed(11)
    net = Network(dt=1.0)
    for name, layer in (("X", Input(shape=(3, 8, 8))), ("H", IFNodes(shape=(20, 8, 8))), ("Y", IFNodes(shape=(24, 8, 8)))):
        net.add_layer(layer, name)
    w = {"H": torch.rand(20, 3, 3, 3, generator=g), "Y": (torch.rand(24, 20, 3, 3, generator=g) - 0.2) * 0.4}
    for src, dst in (("X", "H"), ("H", "Y")):
        net.add_connection(Conv(net.layers[src], net.layers[dst], 3, padding=1, w=w[dst], b=torch.randn(len(w[dst]), generator=g),
                                prop_auto=ask and dst == "Y"), src, dst)
        net.add_monitor(Monitor(net.layers[dst], ["s"], time=T), dst)
    net = net.to(DEV)
    inp = (np.random.default_rng(2).random((T, B, 3, 8, 8)) < 0.3).astype(np.uint8)
    step, ras = T // pieces, {"H": [], "Y": []}
    for p in range(pieces):
        net.run({"X": torch.from_numpy(inp[p * step:(p + 1) * step]).to(DEV)}, time=step)
        assert net.last_plan == "generic"
        for name in ras:
            ras[name].append(net.monitors[name].get("s").cpu().numpy().reshape(-1, B, net.layers[name].n)[-step:].copy())
    out = {"s" + k: np.concatenate(v).astype(np.uint8) for k, v in ras.items()}
    out.update({"v" + k: net.layers[k].v.cpu().numpy().view(np.uint32) for k in ras})
    return out, net.prop_stats()


def test_network_twins_differ_only_in_the_route():
    (plain, st_plain), (asked, st_asked), (halves, st_halves) = _net_run(False, 1), _net_run(True, 1), _net_run(True, 2)
    assert plain["sH"].sum() > 0 and plain["sY"].sum() > 0 and plain["sY"].mean() < 0.9
    for k in plain:
        np.testing.assert_array_equal(plain[k], asked[k], err_msg=k)
        np.testing.assert_array_equal(asked[k], halves[k], err_msg=k)
    zeros = {"matrix_tiles": 0, "event_tiles": 0}
    assert st_plain == {("X", "H"): zeros, ("H", "Y"): zeros} and st_asked[("X", "H")] == zeros and st_halves == st_asked
    assert st_asked[("H", "Y")]["matrix_tiles"] > 0 and st_asked[("H", "Y")]["event_tiles"] == 0
