"""Per-neuron (tensor-valued) node parameters on the device: snn_layer_desc.pv and the per-neuron instances of the step kernels
(include/snnhip.h f10), against the reference-generated fixtures of tests/golden/make_golden_pervec.py, bit for bit, on the generic
plan; hand-stepped layers and the acceptance matrix against the host path (itself pinned to the same fixtures by
tests/test_pervec_host.py)."""
import numpy as np
import pytest
import torch

import pervec_cases as PC
from dt_cases import run_time
from test_pervec_host import _bits, check_snapshots, gold, matrix, ns

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def few_host_threads():
    """(the checker of some tests is the plain-PyTorch host path: torch's default thread count on a many-core GPU box makes its
    small operators slow)"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(4, n))
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_device_reproduces_reference_fixture_twice(name):
    """Every case against its fixture, and the whole case a second time from a fresh state on the same network object (its cached
    vectors and scratch are those of the first pass).

    The derived buffers come from the fixture: made with torch.exp on another host, trace_decay of case (a) differed in its last
    bit for one neuron (profiles/NOTES_pervec.md)."""
    from bindsnet_amd.network.monitors import Monitor
    c = PC.CASES[name]
    net = PC.build(ns(), name)
    PC.load_derived(net, gold(name))                      # (the reference's own decay buffers: see pervec_cases.load_derived)
    net.to(DEV)
    first = PC.run_case(net, name, Monitor, device=DEV)
    assert net.last_plan == "generic"
    check_snapshots(name, first)
    if c["kind"] in ("dc", "alif"):                       # theta is not reset between inputs: a second pass needs it back at zero
        net.layers["Y"].theta.zero_()
    if c.get("postpre"):
        net.connections[("X", "Y")].pipeline[0].value.data.copy_(torch.from_numpy(_w0(name)).to(DEV))
    again = PC.run_case(net, name, Monitor, device=DEV)
    assert net.last_plan == "generic"
    check_snapshots(name, again)


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_second_input_runs_on_the_kept_descriptors(name, monkeypatch):
    """Every case with ONE monitor kept on the network, so that nothing is assigned to any of its objects between the two inputs:
    the second input must run on the descriptor arrays the first built (per-neuron pointers included), not on rebuilt ones, and
    give the fixture's second snapshot."""
    from bindsnet_amd.network.monitors import Monitor
    from bindsnet_amd.network.network import Network
    c = PC.CASES[name]
    net = PC.build(ns(), name)
    PC.load_derived(net, gold(name))
    mon = Monitor(net.layers["Y"], ["s"], time=c["T"])
    net.add_monitor(mon, name="Y_mon")
    net.to(DEV)
    builds = []
    real = Network._build_descriptors
    monkeypatch.setattr(Network, "_build_descriptors", lambda self, *a, **k: builds.append(1) or real(self, *a, **k))
    Y, kept, snaps = net.layers["Y"], [], []
    if c["kind"] == "izh":
        # IzhikevichNodes.reset_state_variables() ASSIGNS u = b * v, as the reference does, and an assignment rebuilds: the same
        # reset written in place (set here, before the first run, being an assignment itself)
        Y.reset_state_variables = lambda: (Y.s.zero_(), Y.x.zero_(), Y.v.fill_(float(Y.rest)), Y.u.copy_(Y.b * Y.v))
    torch.manual_seed(100 + c["seed"])
    for r in range(c["n_in"]):
        net.run({"X": torch.from_numpy(PC.inputs(name, r)).to(DEV)}, time=run_time(c["T"], c.get("dt", 1.0)))
        assert net.last_plan == "generic"
        kept.append(net.__dict__["_run_cache"])
        snaps.append(PC.snapshot(net, name, mon.get("s").cpu().numpy().reshape(c["T"], c["B"], -1).astype(np.uint8)))
        net.reset_state_variables()
    assert c["n_in"] == 2 and len(builds) == 1 and kept[1] is kept[0] and kept[0] is not None, "the second input rebuilt the descriptors"
    check_snapshots(name, snaps)


def _w0(name):
    return PC.weights(PC.build(ns(), name)).detach().numpy().copy()


@pytest.mark.parametrize("name", ["a", "b3", "d", "e_if", "e_boosted", "e_clif", "e_mcp", "e_izh", "f"])
def test_hand_stepped_layer_equals_the_host_path(name):
    """layer.forward(x) on a device layer takes the same path through ops: one layer of each class (and the Input layer of (f))
    stepped by hand on both sides."""
    c = PC.CASES[name]
    B, n = c["B"], int(np.prod(c["shape"]))
    lo, hi = {"lif": (0.0, 6.0), "dc": (0.0, 6.0), "alif": (0.0, 6.0), "if": (-2.0, 5.0), "boosted": (-1.0, 5.0), "clif": (-0.5, 2.0),
              "mcp": (-0.5, 1.5), "izh": (0.0, 12.0)}[c["kind"]]
    cur = (lo + (hi - lo) * np.random.default_rng(1).random((20, B, *c["shape"]), dtype=np.float32)).astype(np.float32)
    spikes = PC.inputs(name, 0)[:20]
    got = {}
    for dev in ("cpu", DEV):
        net = PC.build(ns(), name)
        layer = net.layers["X"] if c.get("input_vec") else net.layers["Y"]
        layer.set_batch_size(B)
        layer.to(dev)
        layer.set_batch_size(B)
        torch.manual_seed(5)
        ss = []
        for t in range(20):
            x = torch.from_numpy(spikes[t].copy() if c.get("input_vec") else cur[t].copy()).to(dev)
            layer.forward(x)
            ss.append(layer.s.cpu().numpy().astype(np.uint8).copy())
        got[dev] = dict(s=np.stack(ss), x=layer.x.cpu().numpy().copy(), rng=torch.get_rng_state().numpy().copy(),
                        **{k: getattr(layer, k).cpu().numpy().copy() for k in ("v", "theta", "i", "u") if isinstance(getattr(layer, k, None), torch.Tensor)})
    assert got["cpu"]["s"].sum() > 0
    for k in got["cpu"]:
        if k in ("s", "rng"):
            np.testing.assert_array_equal(got[DEV][k], got["cpu"][k], err_msg=k)
        else:
            np.testing.assert_array_equal(_bits(got[DEV][k]), _bits(got["cpu"][k]), err_msg=k)


def test_in_place_edit_of_a_vector_is_seen_by_the_next_run():
    """Four runs with one monitor kept on the network: the second runs on the kept descriptors of the first, the third follows an
    in-place edit of a parameter tensor, the fourth one of the derived buffer the kernels read."""
    from bindsnet_amd.network.monitors import Monitor
    name = "e_boosted"
    c = PC.CASES[name]
    x = torch.from_numpy(PC.inputs(name, 0))
    out = {}
    for dev in ("cpu", DEV):
        net = PC.build(ns(), name)
        mon = Monitor(net.layers["Y"], ["s"], time=c["T"])
        net.add_monitor(mon, "Y")
        net.to(dev)
        Y = net.layers["Y"]
        rasters = []
        for step in range(4):
            net.run({"X": x.to(dev)}, time=c["T"])
            rasters.append(mon.get("s").cpu().numpy().astype(np.uint8).copy())
            net.reset_state_variables()
            if step == 1:
                Y.thresh[::2] += 4.0                        # in place: no attribute is assigned
            if step == 2:
                Y.decay.mul_(0.9)                           # the derived buffer the kernels read
        out[dev] = rasters
    assert np.array_equal(out["cpu"][0], out["cpu"][1])
    assert not np.array_equal(out["cpu"][1], out["cpu"][2]) and not np.array_equal(out["cpu"][2], out["cpu"][3])
    for a, b in zip(out[DEV], out["cpu"]):
        np.testing.assert_array_equal(a, b)


def test_in_place_edit_of_a_vector_held_as_a_copy():
    """A strided tensor is brought into the kernels' layout once and kept: an in-place edit of the original must replace the copy."""
    x = torch.from_numpy(PC.matrix_input(3, 0))
    out = {}
    for dev in ("cpu", DEV):
        net = PC.matrix_net(ns(), "IFNodes:thresh")
        net.to(dev)
        Y = net.layers["Y"]
        Y.thresh = torch.stack([Y.thresh, Y.thresh], 1)[:, 0]          # same values, stride 2
        assert not Y.thresh.is_contiguous()
        vs = []
        for step in range(2):
            net.run({"X": x.to(dev)}, time=PC.M_T)
            vs.append(Y.v.cpu().numpy().copy())
            net.reset_state_variables()
            Y.thresh.sub_(6.0)
        out[dev] = vs
    assert not np.array_equal(out["cpu"][0], out["cpu"][1])
    for a, b in zip(out[DEV], out["cpu"]):
        np.testing.assert_array_equal(_bits(a), _bits(b))


def test_diehl_and_cook_model_with_tensor_theta_plus():
    """DiehlAndCook2015 with a tensor theta_plus runs on the generic plan; with the default scalar it keeps the fused plan.  With
    the same value for every neuron the two compute the same bits."""
    from bindsnet_amd import synth
    from bindsnet_amd.models import DiehlAndCook2015
    N, T, B = 100, 50, 1
    spikes = torch.from_numpy(synth.spike_train(50, T, B, 784)).view(T, B, 1, 28, 28)
    out = {}
    for kind, theta_plus in (("scalar", 0.05), ("tensor", torch.full((N,), 0.05))):
        torch.manual_seed(0)
        net = DiehlAndCook2015(n_inpt=784, n_neurons=N, exc=22.5, inh=120, dt=1.0, norm=78.4, theta_plus=theta_plus, inpt_shape=(1, 28, 28))
        net.connections[("X", "Ae")].pipeline[0].value.data.copy_(torch.from_numpy(synth.weights_q12(10, 784, N)))
        net.to(DEV)
        torch.manual_seed(7)
        net.run({"X": spikes.to(DEV)}, time=T)
        out[kind] = dict(plan=net.last_plan, theta=net.layers["Ae"].theta.cpu().numpy(), v=net.layers["Ae"].v.cpu().numpy(),
                         W=net.connections[("X", "Ae")].pipeline[0].value.detach().cpu().numpy())
    assert out["tensor"]["plan"] == "generic"
    assert out["scalar"]["plan"].startswith("dc2015-"), out["scalar"]["plan"]
    assert out["scalar"]["theta"].max() > 0, "vacuous: no spike"
    for k in ("theta", "v", "W"):
        np.testing.assert_array_equal(_bits(out["tensor"][k]), _bits(out["scalar"][k]), err_msg=k)


def test_wrong_length_tensor_is_refused():
    from bindsnet_amd.network.nodes import BoostedLIFNodes, DiehlAndCookNodes
    for layer in (BoostedLIFNodes(n=10, tc_decay=torch.full((7,), 100.0)), DiehlAndCookNodes(shape=[2, 5], theta_plus=torch.full((10,), 0.05))):
        layer.compute_decays(1.0)
        layer.to(DEV)
        layer.set_batch_size(2)
        with pytest.raises(ValueError):
            layer.forward(torch.zeros(2, *layer.shape, device=DEV))
    net = PC.matrix_net(ns(), "IFNodes:thresh")
    net.layers["Y"].thresh = torch.zeros(7)
    net.to(DEV)
    with pytest.raises(ValueError):
        net.run({"X": torch.zeros(4, 1, PC.M_SRC, dtype=torch.uint8, device=DEV)}, time=4)


@pytest.mark.parametrize("pair", matrix()[1])
def test_device_refuses_what_the_reference_refuses(pair):
    """... with NotImplementedError, before the run changes any state."""
    net = PC.matrix_net(ns(), pair)
    net.to(DEV)
    x = torch.from_numpy(PC.matrix_input(3, 0)).to(DEV)
    with pytest.raises(NotImplementedError):
        net.run({"X": x}, time=PC.M_T)
    Y = net.layers["Y"]
    assert not Y.s.any() and (Y.x == 0).all()


@pytest.mark.parametrize("pair", matrix()[0])
def test_device_runs_what_the_reference_runs(pair):
    """Every accepted pair on the device against the host path, bit for bit."""
    host, dev = PC.matrix_run(ns(), pair), PC.matrix_run(ns(), pair, device=DEV)
    for h, d in zip(host, dev):
        for a, b in zip(h[:3], d[:3]):
            np.testing.assert_array_equal(_bits(b), _bits(a))
        np.testing.assert_array_equal(d[3], h[3])
