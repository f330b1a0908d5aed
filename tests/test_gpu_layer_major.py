"""The layer-major plan on the device (Network.layer_major, network/layer_major.py): snn_run_conv2d_sif_f32 -- a Conv2dConnection and its
SubtractiveResetIFNodes over the whole run in one launch -- and the time-chunked route with snn_sif_scan, against a plain float64
reference (weights on a 1/64 grid: every partial sum exact, so equality is exact) and, with randn weights, bit for bit against the
generic plan, after one run and after a second run without a reset."""
import numpy as np
import pytest
import torch

from layer_major_cases import build, reference, spike_input, weights

pytestmark = pytest.mark.gpu

# name: (spec, T, B, options).  Kernel 1 is every "conv" fed spike bytes; its shapes are the smallest at which it can go wrong.
# "stream": a 5x5 bank of 97 -> 5 channels pads to 25 * 112 = 2800 terms = 44 slabs x 4 KiB = 176 KiB per channel group, beyond the 150 KiB
# the kernel may ask for, so the weights stream through two slabs every step (run_conv2d_sif_takes == 2, asserted); the others stay resident.
CASES = {
    "c3_5_5x5": (((3, 5, 5), [("conv", 5, 3, 1, 1)]), 7, 3, {}),
    "c17_16_9x7_refrac": (((17, 9, 7), [("conv", 16, 3, 1, 1)]), 7, 1, dict(refrac=2)),
    "c32_20_9x7_lbound": (((32, 9, 7), [("conv", 20, 3, 1, 1)]), 2, 3, dict(lbound=-0.25)),
    "stride2": (((17, 9, 7), [("conv", 20, 3, 2, 1)]), 7, 3, dict(refrac=2)),
    "k1_T1": (((32, 5, 5), [("conv", 5, 1, 1, 0)]), 1, 1, {}),
    "stream": (((97, 5, 5), [("conv", 5, 5, 1, 2)]), 2, 1, dict(takes=2, density=0.1)),
    "byte2_traces": (((17, 9, 7), [("conv", 20, 3, 1, 1), ("conv", 5, 3, 1, 1)]), 7, 3, dict(two=True, traces=True)),
    "stack_bytes": (((3, 9, 9), [("conv", 20, 3, 1, 1), ("conv", 16, 3, 1, 1), ("pool",), ("fc", 12), ("fc", 5)]), 7, 3, {}),
    "stack_analog": (((3, 9, 9), [("conv", 20, 3, 1, 1), ("conv", 16, 3, 1, 1), ("pool",), ("fc", 12), ("fc", 5)]), 7, 3, dict(analog=True)),
}


def run_twice(net, xs):
    """Two runs without a reset; per run: every layer's train, then every layer's state."""
    from bindsnet_amd.network.monitors import Monitor
    out = []
    for x in xs:
        mons = {l: Monitor(layer, ["s"], time=x.shape[0]) for l, layer in net.layers.items() if l != "0"}
        for l, m in mons.items():
            net.add_monitor(m, "m" + l)
        net.run({"0": x.to("cuda")}, time=x.shape[0])
        trains = [mons[l].get("s").to(torch.uint8).cpu() for l in sorted(mons, key=int)]
        state = [{k: getattr(net.layers[l], k).detach().float().cpu().clone() for k in ("s", "v", "refrac_count", "x", "summed")
                  if isinstance(getattr(net.layers[l], k, None), torch.Tensor)} for l in sorted(mons, key=int)]
        out.append((trains, state, net.last_plan))
        for l in mons:
            del net.monitors["m" + l]
    return out


def inputs_of(name):
    spec, T, B, opt = CASES[name]
    xs = [spike_input(spec, T, B, seed, opt.get("density", 0.3), opt.get("analog", False)) for seed in (11, 12)]
    if opt.get("two"):
        xs[0][min(2, T - 1), B - 1, 1, 2, 3] = 2                  # one byte above 1: that workgroup's next step takes the scalar body
    return xs


def options(opt):
    return dict(refrac=opt.get("refrac", 0), lbound=opt.get("lbound"), traces=opt.get("traces", False))


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_float64_reference(name):
    from bindsnet_amd import ops
    spec, T, B, opt = CASES[name]
    ws, xs = weights(spec, 5, grid=True), inputs_of(name)
    if "takes" in opt:
        op = spec[1][0]
        assert ops.run_conv2d_sif_takes(T, B, *spec[0], op[1], op[2], op[2], op[3], op[4]) == opt["takes"]
    net = build(spec, ws, B, True, **options(opt)).to("cuda")
    state, fired = {}, 0
    for x, (trains, st, plan) in zip(xs, run_twice(net, xs)):      # (the second run starts from a non-zero frame and state)
        want = reference(spec, ws, x, state, opt.get("refrac", 0), opt.get("lbound"))
        assert plan == "layer-major"
        fired += sum(int(w.sum()) for w in want)
        for k, (got, w) in enumerate(zip(trains, want)):
            assert torch.equal(got.reshape(w.shape), w), f"train of layer {k + 1}"
            assert torch.equal(st[k]["v"].double().reshape(state["v"][k].shape), state["v"][k]), f"v of layer {k + 1}"
            assert torch.equal(st[k]["refrac_count"].double().reshape(state["rc"][k].shape), state["rc"][k]), f"refrac_count of layer {k + 1}"
        assert torch.equal(st[-1]["summed"].double().reshape(state["summed"].shape), state["summed"])
    assert fired > 0                                               # (at T = 1 the first run sees only the zero start frame)


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_generic_plan_bit_for_bit(name):
    spec, T, B, opt = CASES[name]
    ws, xs = weights(spec, 6, grid=False), inputs_of(name)
    runs = [run_twice(build(spec, ws, B, lm, **options(opt)).to("cuda"), xs) for lm in (True, False)]
    for (trains, st, plan), (trains0, st0, plan0) in zip(*runs):
        assert (plan, plan0) == ("layer-major", "generic")
        for k in range(len(trains)):
            assert torch.equal(trains[k], trains0[k]), f"train of layer {k + 1}"
            assert st[k].keys() == st0[k].keys()
            for key in st[k]:
                assert np.array_equal(st[k][key].numpy().view(np.uint32), st0[k][key].numpy().view(np.uint32)), f"{key} of layer {k + 1}"
    assert sum(int(t.sum()) for trains0, _, _ in runs[1] for t in trains0) > 0


def with_maxpool(net):
    from bindsnet_amd.conversion import PassThroughNodes
    from bindsnet_amd.network.topology import MaxPool2dConnection
    src = net.layers["1"]
    net.add_layer(PassThroughNodes(shape=(src.shape[0], src.shape[1] // 2, src.shape[2] // 2)), "2")
    net.add_connection(MaxPool2dConnection(src, net.layers["2"], kernel_size=2, stride=2, decay=1), "1", "2")


def with_v_monitor(net):
    from bindsnet_amd.network.monitors import Monitor
    net.add_monitor(Monitor(net.layers["1"], ["v"], time=7), "v1")


@pytest.mark.parametrize("extra", (with_maxpool, with_v_monitor))
def test_a_graph_that_does_not_qualify_runs_the_generic_plan(extra):
    spec, T, B, _ = CASES["c17_16_9x7_refrac"]
    ws, x = weights(spec, 6, grid=False), spike_input(spec, T, B, 11).to("cuda")
    seen = []
    for lm in (True, False):
        net = build(spec, ws, B, lm, extra=extra).to("cuda")
        net.run({"0": x}, time=T)
        seen.append((net.last_plan, net.layers["1"].v.cpu().numpy().view(np.uint32), net.layers["1"].s.cpu().numpy()))
    assert seen[0][0] == seen[1][0] == "generic"
    assert np.array_equal(seen[0][1], seen[1][1]) and np.array_equal(seen[0][2], seen[1][2])
