"""bindsnet.conversion on the HOST: the package's host path pinned to the reference-generated fixtures of
tests/golden/make_golden_conversion.py (cases in tests/conversion_cases.py).

Dyadic cases (every sum exact in f32): every field bit for bit.  Float cases: rasters, refrac_count and traces bit for bit, v and
summed within the spreads the generator measured against the stated order and stored in the fixture (`Connection.compute` is an
MKL sgemm in the reference and here, whose order belongs to the machine); the stated order itself is held to the same fixture, so
that the GPU tests can pin the device to it bit for bit.  Then what ann_to_snn builds (names, keys, shapes, parameters), the
normalisation on integer-valued models, the classes' buffers and semantics, and everything that raises."""
import io
import json
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases
import conversion_cases as CC


def _ns():
    from bindsnet_amd import conversion
    from bindsnet_amd.network import Network, nodes, topology
    from bindsnet_amd.network.monitors import Monitor
    return CC.ns_from(nodes, topology, Network, Monitor, conversion)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1)


def gold(name):
    return cases.gold("conversion_" + name)


def params_of(name, g):
    return [g[f"param{k}"] for k in range(sum(f.startswith("param") and f != "params_sha" for f in g.files))] if CC.stores_params(name) else None


def check_snapshots(name, snaps, g, first=0, exact=None):
    """The snapshots of run_case / stated_run against the fixture.  exact: v and summed bit for bit (default: the dyadic family);
    otherwise within the fixture's v_spread / summed_spread."""
    exact = name not in CC.FLOAT if exact is None else exact
    seen = 0
    for i, s in enumerate(snaps):
        r = first + i
        for k, v in s.items():
            if k.endswith("_vrec") or k.endswith("_margin"):
                continue
            ref = g[f"r{r}_{k}"]
            seen += 1
            if k.endswith("_raster"):
                want = cases.unpack(ref, v.shape)
                assert 0 < int(want.sum()) < want.size, "a raster that is all zeros or all ones checks nothing"
                assert np.array_equal(np.asarray(v, np.uint8), want), f"case {name} input {r}: {k} differs ({int(np.asarray(v).sum())} vs {int(want.sum())} spikes)"
            elif not exact and (k.endswith("_v") or k.endswith("_summed")):
                spread = float(g["summed_spread" if k.endswith("_summed") else "v_spread"])
                err = float(np.abs(np.asarray(v, np.float64).reshape(-1) - ref.astype(np.float64).reshape(-1)).max())
                assert err <= spread, f"case {name} input {r}: {k} is {err:.3g} from the reference, the measured spread is {spread:.3g}"
            else:
                got, want = _bits(v), _bits(ref)
                assert got.size == want.size and np.array_equal(got, want), f"case {name} input {r}: {k} differs at {np.flatnonzero(got != want)[:5]}"
    assert seen > 0


def test_reference_names_resolve():
    import bindsnet
    from bindsnet.conversion import (ConstantPad2dConnection, FeatureExtractor, PassThroughNodes, Permute, PermuteConnection,  # noqa: F401
                                     SubtractiveResetIFNodes, ann_to_snn, data_based_normalization)
    from bindsnet_amd import _lib, conversion
    assert bindsnet.conversion is conversion and "conversion" in bindsnet._SUBPACKAGES
    assert set(conversion.__all__) == {"Permute", "FeatureExtractor", "data_based_normalization", "ann_to_snn", "SubtractiveResetIFNodes",
                                       "PassThroughNodes", "PermuteConnection", "ConstantPad2dConnection"}
    assert conversion.PermuteConnection._kind == _lib.CONN_PERMUTE == 8 and conversion.ConstantPad2dConnection._kind == _lib.CONN_PAD == 9
    assert (_lib.LAYER_SIF, _lib.LAYER_PASS) == (10, 11)
    for cls in (conversion.PermuteConnection, conversion.ConstantPad2dConnection):
        assert cls._rules == {"NoOp"} and cls._takes_mask is False and cls._multi_device is False


@pytest.mark.parametrize("name", CC.CASES)
def test_host_path_equals_reference(name):
    g = gold(name)
    ns = _ns()
    net = CC.build(ns, name, params=params_of(name, g), seed=int(g["seed"]))        # (training mode: this package's connections run in it)
    snaps = CC.run_case(ns, net, name)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps, g)


@pytest.mark.parametrize("name", CC.CASES)
def test_stated_order_equals_reference(name):
    """Half 2 of the float contract (and, for the dyadic family, that the stated order is exact too)."""
    g = gold(name)
    snaps = CC.stated_run(name, params=params_of(name, g), seed=int(g["seed"]))
    check_snapshots(name, snaps, g)
    if name in CC.FLOAT:
        margin = min(v for s in snaps for k, v in s.items() if k.endswith("_margin"))
        assert margin >= CC.MARGIN * float(g["v_spread"]), (margin, float(g["v_spread"]))
        assert margin == pytest.approx(float(g["least_margin"]), rel=1e-3)


@pytest.mark.parametrize("name", ["g_pad_spiking", "mlp_dy_b3", "cnn_dy", "step_n257"])
def test_two_half_runs_equal_one(name):
    g = gold(name)
    ns = _ns()
    net = CC.build(ns, name, seed=int(g["seed"]))
    check_snapshots(name, CC.run_case(ns, net, name, halves=True, count=1), g)


@pytest.mark.parametrize("name", list(CC.NETS))
def test_ann_to_snn_builds_what_the_reference_builds(name):
    g = gold(name)
    ns = _ns()
    net = CC.build(ns, name, seed=int(g["seed"]))          # (a `data` case normalises for itself here)
    layers = [(k, type(l).__name__, [int(x) for x in l.shape]) for k, l in net.layers.items()]
    conns = [(list(k), type(c).__name__) for k, c in net.connections.items()]
    assert json.loads(str(g["layers"])) == [list(x) for x in layers]
    assert json.loads(str(g["connections"])) == [list(x) for x in conns]
    if not CC.stores_params(name):                         # (float activations in the normalisation: the last bits belong to the machine)
        assert json.loads(str(g["params_sha"])) == [CC.sha(a) for a in CC.net_params(net)]
    last = list(net.layers.values())[-1]
    assert last.sum_input and last.summed.shape == last.v.shape
    for l in net.layers.values():
        if hasattr(l, "refrac_count"):
            assert float(l.thresh) == 1.0 and float(l.reset) == 0.0 and int(l.refrac) == 0 and (l.sum_input is (l is last))
    for c in net.connections.values():
        if type(c).__name__ == "Connection":
            assert tuple(c.w.shape) == (c.source.n, c.target.n) and c.b is not None
        if type(c).__name__ == "MaxPool2dConnection":
            assert c.decay == 1


def test_ann_to_snn_copies_the_model_and_warns_without_data():
    from bindsnet_amd.conversion import ann_to_snn
    ann = nn.Sequential(nn.Linear(5, 4), nn.ReLU(), nn.Linear(4, 3))
    with pytest.warns(RuntimeWarning, match="Data is None"):
        net = ann_to_snn(ann, (5,))
    w = net.connections[("0", "1")].w
    assert torch.equal(w, ann[0].weight.t()) and w.data_ptr() != ann[0].weight.data_ptr()
    ann2, data, shape = CC.norm_case("cnn")
    before = [p.detach().clone() for p in ann2.parameters()]
    ann_to_snn(ann2, shape, data=data)
    assert all(torch.equal(a, b) for a, b in zip(before, ann2.parameters())), "the caller's model was rescaled"


@pytest.mark.parametrize("kind", ["mlp", "cnn"])
def test_normalisation_equals_reference(kind):
    from bindsnet_amd.conversion import data_based_normalization
    g = cases.gold("conversion_norm")
    ann, data, _ = CC.norm_case(kind)
    assert data_based_normalization(ann, data) is ann
    for k, p in enumerate(ann.parameters()):
        assert not p.requires_grad
        assert np.array_equal(_bits(p.detach().numpy()), _bits(g[f"{kind}_{k}"])), f"{kind} parameter {k}"


# ---- what raises, and what this package does on purpose where the reference cannot construct the class at all -----------------------
# call -> this package's outcome where it is NOT the recorded one, with the reason
DEVIATIONS = {
    "pad_asymmetric": "RuntimeError",      # runs in the reference (the connection hands the 66 padded elements on); here the 48-neuron target of the helper's quirk does not fit the weights: refused at the first step's matmul, before any state changes
    "pad_symmetric": "ok",                 # the reference's NoOp fails on the missing `w` in training mode; this package runs such connections in training mode
    "node_type_if": "NotImplementedError",         # sum_input=True on another class
    "sum_input_on_input": "NotImplementedError",   # (tests/test_abi.py pins it)
}


def test_raises_as_recorded():
    rec = json.load(open(os.path.join(cases.GOLD, "conversion_raises.json")))
    assert rec["construct_PermuteConnection"]["reference"] == rec["construct_ConstantPad2dConnection"]["reference"] == "TypeError"
    ns = _ns()
    for call in CC.CALLS:
        want = DEVIATIONS.get(call, rec[call]["concrete"])
        assert CC.outcome(ns, call) == want, (call, CC.outcome(ns, call), rec[call])


def test_sum_input_only_on_subtractive_reset_nodes():
    from bindsnet_amd.conversion import PassThroughNodes, SubtractiveResetIFNodes
    from bindsnet_amd.network import nodes
    for cls in (nodes.Input, nodes.IFNodes, nodes.LIFNodes, nodes.McCullochPitts, nodes.DiehlAndCookNodes, PassThroughNodes):
        with pytest.raises(NotImplementedError):
            cls(n=3, sum_input=True)
    layer = SubtractiveResetIFNodes(n=3, traces=True, sum_input=True)
    assert list(layer.state_dict()) == ["s", "x", "tc_trace", "trace_scale", "trace_decay", "summed", "reset", "thresh", "refrac", "v", "refrac_count"]
    assert layer.refrac.dtype == torch.int64 and layer.lbound is None
    layer.compute_decays(1.0)
    layer.set_batch_size(2)
    assert layer.summed.shape == (2, 3) and layer.summed.dtype == torch.float32 and layer.refrac_count.dtype == torch.float32
    assert "summed" not in SubtractiveResetIFNodes(n=3).state_dict()


def test_step_semantics_and_pickle():
    from bindsnet_amd.conversion import SubtractiveResetIFNodes
    from bindsnet_amd.network import Network
    net = Network(dt=1.0, batch_size=1)
    layer = SubtractiveResetIFNodes(n=4, thresh=1.0, reset=0.25, refrac=2, lbound=-0.5, sum_input=True)
    net.add_layer(layer, name="Y")
    assert torch.equal(layer.v, torch.full((1, 4), 0.25))
    cur = torch.tensor([[[1.0, 0.5, -2.0, 3.0]], [[1.0, 0.5, 0.0, 0.0]]])
    net.run({"Y": cur.clone()}, time=2)
    # step 0: v = .25 + x -> [1.25, .75, -1.75, 3.25]; spikes 0 and 3 keep v - thresh; lbound lifts neuron 2.  Step 1: 0 and 3 are
    # refractory (v stays, and 3 spikes again from what it kept), 1 integrates to the threshold
    assert layer.v.tolist() == [[0.25, 0.25, -0.5, 1.25]] and layer.s.tolist() == [[False, True, False, True]]
    assert layer.refrac_count.tolist() == [[1.0, 2.0, 0.0, 2.0]] and layer.summed.tolist() == [[2.0, 1.0, -2.0, 3.0]]
    buf = io.BytesIO()
    pickle.dump(net, buf)
    buf.seek(0)
    back = pickle.load(buf)
    assert torch.equal(back.layers["Y"].summed, layer.summed) and back.layers["Y"].sum_input
    net.reset_state_variables()
    assert torch.equal(layer.v, torch.full((1, 4), 0.25)) and not layer.summed.any() and not layer.refrac_count.any() and not layer.s.any()


def test_pass_through_semantics():
    from bindsnet_amd.conversion import PassThroughNodes
    layer = PassThroughNodes(shape=[2, 3], traces=True)
    layer.compute_decays(1.0)
    layer.set_batch_size(2)
    assert layer.v.shape == (2, 3) and not layer.v.any()
    x = torch.rand(2, 2, 3)
    layer.forward(x)
    assert layer.s is x and layer.s.dtype == torch.float32 and not layer.x.any() and not layer.v.any()       # no trace: the base class is never reached
    layer.x.fill_(0.5)
    layer.reset_state_variables()
    assert not layer.s.any() and float(layer.x.min()) == 0.5                                                # zeroes `s` only


def test_connections_by_hand_and_their_refusals():
    from bindsnet_amd.conversion import ConstantPad2dConnection, PassThroughNodes, PermuteConnection
    from bindsnet_amd.learning import PostPre
    from bindsnet_amd.network import Network, nodes
    from bindsnet_amd.network.monitors import Monitor
    X, P = nodes.Input(shape=(2, 3, 5), traces=True), PassThroughNodes(shape=[5, 2, 3], traces=True)
    perm = PermuteConnection(X, P, dims=(0, 3, 1, 2))
    s = torch.rand(4, 2, 3, 5) < 0.5
    out = perm.compute(s)
    assert out.dtype == torch.float32 and torch.equal(out, s.permute(0, 3, 1, 2).float()) and not hasattr(perm, "w")
    pad = ConstantPad2dConnection(X, PassThroughNodes(shape=[2, 6, 8]), padding=(1, 2, 2, 1))
    assert torch.equal(pad.compute(s), torch.nn.functional.pad(s, (1, 2, 2, 1)).float())
    pad.normalize()
    pad.update(learning=True)
    # the device geometry: pure host arithmetic, so what it refuses is checked here too
    arrays, shape = perm._geometry()
    assert shape == (5, 2, 3) and list(arrays[2]) == [1, 15, 5] and list(arrays[3]) == [0, 0, 0]
    arrays, shape = pad._geometry()
    assert shape == (2, 6, 8) and list(arrays[1]) == [2, 3, 5] and list(arrays[2]) == [15, 5, 1] and list(arrays[3]) == [0, 2, 1]
    with pytest.raises(NotImplementedError, match="dims"):
        PermuteConnection(X, P, dims=(1, 0, 2, 3))._geometry()
    with pytest.raises(NotImplementedError, match="dimensions"):
        PermuteConnection(nodes.Input(shape=(2, 2, 2, 2)), P, dims=(0, 1, 2, 3, 4))._geometry()
    with pytest.raises(RuntimeError):
        PermuteConnection(X, P, dims=(0, 2, 1))._geometry()
    with pytest.raises(RuntimeError, match="shape"):
        PermuteConnection(X, P, dims=(0, 2, 3, 1))._checked_geometry()           # (3, 5, 2) is not the target's (5, 2, 3)
    with pytest.raises(NotImplementedError, match="negative"):
        ConstantPad2dConnection(X, P, padding=(1, -1, 0, 0))._geometry()
    with pytest.raises(NotImplementedError, match="4-tuple"):
        ConstantPad2dConnection(X, P, padding=(1, 1))._geometry()
    with pytest.raises(RuntimeError, match="shape"):
        ConstantPad2dConnection(X, P, padding=(1, 1, 1, 1))._checked_geometry()
    # a rule other than NoOp, Dales_rule, a mask, a monitor
    with pytest.raises(NotImplementedError):
        PermuteConnection(X, P, dims=(0, 3, 1, 2), update_rule=PostPre, nu=1e-2)
    with pytest.raises(NotImplementedError):
        ConstantPad2dConnection(X, P, padding=(0, 0, 0, 0), Dales_rule=torch.ones(2))
    net = Network(dt=1.0, batch_size=1)
    net.add_layer(X, name="X")
    net.add_layer(P, name="P")
    net.add_connection(perm, "X", "P")
    x = (torch.rand(3, 1, 2, 3, 5) < 0.5).byte()
    before = torch.get_rng_state()
    with pytest.raises(NotImplementedError, match="mask"):
        net.run({"X": x}, time=3, masks={("X", "P"): torch.ones(30, 30)})
    net.add_monitor(Monitor(perm, ["dims"], time=3), name="m")
    with pytest.raises(NotImplementedError, match="monitor"):
        net.run({"X": x}, time=3)
    assert not X.x.any() and torch.equal(torch.get_rng_state(), before), "a refused run changed state"
    # what a PassThroughNodes layer refuses on the device, asked by Network.run there
    from bindsnet_amd.network.topology import Connection, MaxPool2dConnection
    assert P._run_refusal("P", [perm], False, False) is None
    assert P._run_refusal("P", [MaxPool2dConnection(X, P, kernel_size=2, decay=1)], False, False) is None
    for args in (([perm, perm], False, False), ([Connection(X, P)], False, False), ([perm], True, False), ([perm], False, True), ([], False, False)):
        assert isinstance(P._run_refusal("P", *args), NotImplementedError)
    from bindsnet_amd.conversion import SubtractiveResetIFNodes
    for name, value in (("thresh", torch.ones(3)), ("reset", torch.zeros(3)), ("refrac", torch.ones(3, dtype=torch.long))):
        layer = SubtractiveResetIFNodes(n=3, **{name: value})
        layer.compute_decays(1.0)
        with pytest.raises(NotImplementedError, match=name):
            layer._params({})
    layer = SubtractiveResetIFNodes(n=3)
    layer.lbound = torch.zeros(3)
    layer.compute_decays(1.0)
    with pytest.raises(NotImplementedError, match="lbound"):
        layer._params({})


def test_multi_device_modes_refuse_by_name():
    from bindsnet_amd import parallel
    g = gold("g_pad_1221")
    net = CC.build(_ns(), "g_pad_1221", seed=int(g["seed"]))
    x = CC.case_inputs("g_pad_1221", 0)
    for mode in (parallel.sharded_run, parallel.exact_run):
        with pytest.raises(NotImplementedError, match="ConstantPad2dConnection|PassThroughNodes|SubtractiveResetIFNodes"):
            mode(net, dict(x), time=CC.GATHER_T)
