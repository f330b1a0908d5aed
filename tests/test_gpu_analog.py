"""A real-valued (analog) Input on the MI355X (include/snnhip.h f17).

* ops.prop_dense_real / ops.prop_conv2d_real / ops.input_step_real over the sweep of tests/analog_cases.py against the numpy stated
  order, bit for bit, outputs in front of and behind guard elements: negative values, values above 1, exact zeros, whole zero
  samples and whole zero sources; with and without bias and `accumulate`.
* The 0/1 invariance: the three operators on float32 zeros and ones against ops.prop_dense / ops.prop_conv2d / ops.input_step on the
  same bytes; whole runs of a converted MLP, a converted CNN and a hand-built graph with masks=, a bias and a norm.
* Every fixture case of tests/golden/make_golden_analog.py through Network.run on the device, on the generic plan.  Dyadic family:
  every field against the REFERENCE's record, bit for bit.  Float family: every field against the stated order bit for bit --
  tests/test_analog_host.py holds the stated order to the reference --, and against the reference's record within the spreads.
* compute() / forward() on device tensors, the Input's float32 `s` monitor, what an unreset `s` does to the next run, and every
  refusal, each before any state changes."""
import numpy as np
import pytest
import torch

import analog_cases as AC
import conversion_cases as CC
from test_analog_host import _ns
from test_gpu_conversion import _gather_net, _refused

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
FILL = 7.5


def _dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def _guarded(shape, prev):
    """A device output of `shape` between GUARD elements of FILL on either side: (view, whole buffer); NaN inside unless `prev`."""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), FILL, dtype=torch.float32, device=DEV)
    flat[GUARD:GUARD + n] = float("nan") if prev is None else torch.from_numpy(prev).reshape(-1).to(DEV)
    return flat[GUARD:GUARD + n].view(*shape), flat


def _intact(flat):
    return bool((flat[:GUARD] == FILL).all()) and bool((flat[-GUARD:] == FILL).all())


def _same(t, want):
    got = t.detach().cpu().numpy()
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ---- the operators ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nin", AC.DENSE_NIN)
def test_dense_real_equals_the_stated_order(nin):
    from bindsnet_amd import ops
    for c in AC.dense_sweep(nin):
        out, flat = _guarded(c["want"].shape, c["prev"])
        ops.prop_dense_real(_dev(c["w"]), _dev(c["x"]), out, bias=_dev(c["b"]), accumulate=c["prev"] is not None)
        what = (nin, c["w"].shape[1], c["x"].shape[0], c["b"] is not None, c["prev"] is not None)
        assert _same(out, c["want"]), what
        assert _intact(flat), what


@pytest.mark.parametrize("img", AC.CONV_IMG)
@pytest.mark.parametrize("cin", AC.CONV_CIN)
def test_conv2d_real_equals_the_stated_order(cin, img):
    from bindsnet_amd import ops
    for c in AC.conv_sweep(cin, img):
        out, flat = _guarded(c["want"].shape, c["prev"])
        ops.prop_conv2d_real(_dev(c["w"]), _dev(c["x"]), out, bias=_dev(c["b"]), stride=c["stride"], pad=c["pad"], accumulate=c["prev"] is not None)
        what = (cin, img, c["w"].shape[2], c["stride"], c["pad"], c["w"].shape[0], c["x"].shape[0])
        assert _same(out, c["want"]), what
        assert _intact(flat), what


def test_conv2d_real_beyond_the_staged_sizes():
    """More taps than the filters' LDS layout takes (Cin * KH * KW > 1024) and images beyond the staged 48 KiB: the L2 paths."""
    from bindsnet_amd import ops
    rng = np.random.default_rng(77)
    for B, cin, img, K, cout in ((2, 129, (6, 5), 3, 9), (2, 3, (70, 66), 3, 4)):
        x, w, b = AC.real_values(rng, B, cin, *img), (rng.standard_normal((cout, cin, K, K)) * 0.1).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
        want = AC.conv2d_real_stated(x, w, b, 1, 1)
        out, flat = _guarded(want.shape, None)
        ops.prop_conv2d_real(_dev(w), _dev(x), out, bias=_dev(b), stride=1, pad=1)
        assert _same(out, want) and _intact(flat), (cin, img)


def test_input_step_real_equals_the_stated_order():
    from bindsnet_amd import ops
    for c in AC.step_sweep():
        T, B, n = c["s"].shape
        x, xflat = _guarded((B, n), c["x0"])
        pv = {"trace_scale": _dev(c["scale"])} if c["mode"] == "pv" else None
        for t in range(T):
            s = _dev(c["s"][t])
            raster, rflat = _guarded((B, n), None)
            ops.input_step_real(s, x, trace_decay=c["decay"], trace_scale=0.0 if pv else float(c["scale"]), additive=c["additive"], raster=raster, pv=pv)
            assert _same(x, c["want"][t]) and _same(raster, c["s"][t]), (n, B, c["mode"], t)
            assert _intact(xflat) and _intact(rflat)
    with pytest.raises(TypeError):
        ops.input_step_real(torch.zeros(1, 4, dtype=torch.uint8, device=DEV), torch.zeros(1, 4, device=DEV))
    with pytest.raises(TypeError):
        ops.prop_dense_real(torch.zeros(4, 4, device=DEV), torch.zeros(1, 4, dtype=torch.uint8, device=DEV), torch.zeros(1, 4, device=DEV))
    with pytest.raises(TypeError):
        ops.prop_conv2d_real(torch.zeros(1, 1, 1, 1, device=DEV), torch.zeros(1, 1, 2, 2, dtype=torch.float64, device=DEV), torch.zeros(1, 1, 2, 2, device=DEV))


def test_operators_on_zeros_and_ones_equal_the_byte_operators():
    from bindsnet_amd import ops
    rng = np.random.default_rng(11)
    for nin, n, B in ((255, 65, 3), (1025, 257, 9), (784, 10, 1), (257, 1, 3)):
        s = torch.from_numpy((rng.random((B, nin)) < 0.3).astype(np.uint8)).to(DEV)
        w, b = torch.from_numpy(rng.standard_normal((nin, n)).astype(np.float32)).to(DEV), torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
        for bias in (None, b):
            want = ops.prop_dense(w, s, torch.full((B, n), 0.5, device=DEV), bias=bias, accumulate=True)
            got = ops.prop_dense_real(w, s.float(), torch.full((B, n), 0.5, device=DEV), bias=bias, accumulate=True)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (nin, n, B)
            want = ops.prop_dense(w, s, torch.empty(B, n, device=DEV), bias=bias)
            got = ops.prop_dense_real(w, s.float(), torch.empty(B, n, device=DEV), bias=bias)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (nin, n, B)
    for B, cin, img, K, stride, pad, cout in ((3, 3, (12, 12), 3, 1, 1, 9), (1, 1, (28, 28), 5, 1, 0, 8), (3, 17, (5, 7), 3, 2, 2, 8), (2, 3, (32, 32), 3, 1, 1, 16)):
        s = torch.from_numpy((rng.random((B, cin, *img)) < 0.3).astype(np.uint8)).to(DEV)
        w, b = torch.from_numpy(rng.standard_normal((cout, cin, K, K)).astype(np.float32)).to(DEV), torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).to(DEV)
        oh, ow = (img[0] + 2 * pad - K) // stride + 1, (img[1] + 2 * pad - K) // stride + 1
        for acc in (False, True):
            want = ops.prop_conv2d(w, s, torch.full((B, cout, oh, ow), 0.25, device=DEV), bias=b, stride=stride, pad=pad, accumulate=acc)
            got = ops.prop_conv2d_real(w, s.float(), torch.full((B, cout, oh, ow), 0.25, device=DEV), bias=b, stride=stride, pad=pad, accumulate=acc)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (cin, img, K, stride, pad, acc)
    for n, B, additive, pv in ((255, 3, False, None), (257, 3, True, None), (257, 1, True, "pv")):
        vec = {"trace_scale": torch.linspace(0.5, 1.5, n, device=DEV)} if pv else None
        xa = torch.from_numpy(rng.standard_normal((B, n)).astype(np.float32)).to(DEV)
        xb = xa.clone()
        for _ in range(4):
            s = torch.from_numpy((rng.random((B, n)) < 0.3).astype(np.uint8)).to(DEV)
            ops.input_step(s, xa, trace_decay=0.875, trace_scale=0.75, additive=additive, pv=vec)
            ops.input_step_real(s.float(), xb, trace_decay=0.875, trace_scale=0.75, additive=additive, pv=vec)
            assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)), (n, B, additive, pv)


def test_compute_and_forward_on_device_tensors():
    ns = _ns()
    rng = np.random.default_rng(3)
    X, Y = ns.Input(n=37, traces=True, traces_additive=True, tc_trace=8.0, trace_scale=0.75), ns.LIFNodes(n=11)
    w, b = rng.standard_normal((37, 11)).astype(np.float32), rng.standard_normal(11).astype(np.float32)
    conn = ns.Connection(X, Y, w=torch.from_numpy(w), b=torch.from_numpy(b)).to(DEV)
    x = AC.real_values(rng, 3, 37)
    assert _same(conn.compute(_dev(x)), AC.dense_real_stated(x, w, b))
    X4, Y4 = ns.Input(shape=(3, 7, 6)), ns.LIFNodes(shape=(5, 7, 6))
    w4, b4 = rng.standard_normal((5, 3, 3, 3)).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    conv = ns.Conv2dConnection(X4, Y4, kernel_size=3, padding=1, w=torch.from_numpy(w4), b=torch.from_numpy(b4)).to(DEV)
    x4 = AC.real_values(rng, 2, 3, 7, 6)
    assert _same(conv.compute(_dev(x4)), AC.conv2d_real_stated(x4, w4, b4, 1, 1))
    X.to(DEV)
    X.set_batch_size(3)
    X.compute_decays(1.0)
    xd, trace = _dev(x), np.zeros((3, 37), np.float32)
    for _ in range(2):
        X.forward(xd)
        trace = AC.input_trace_stated(trace, x, X.trace_decay.cpu().numpy(), np.float32(0.75), True)
    assert X.s.data_ptr() == xd.data_ptr() and X.s.dtype == torch.float32       # aliased, not copied
    assert _same(X.x, trace)


# ---- whole runs -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", AC.CASES)
def test_device_reproduces_fixture(name):
    g = AC.gold(name)
    ns = _ns()
    net = AC.build(ns, name, seed=int(g["seed"])).to(DEV)
    plans = []
    snaps = AC.run_case(ns, net, name, device=DEV, check=lambda n: plans.append(n.last_plan))
    assert plans and set(plans) == {"generic"}
    assert all(int(v.sum()) > 0 for s in snaps for k, v in s.items() if k.endswith("_raster")), "an empty raster: the kernels were not reached"
    AC.check_snapshots(name, snaps, g)                       # dyadic: bit for bit; float: rasters, refrac_count, traces exact, v and summed within the spreads
    if name in AC.FLOAT:                                     # half 1: the stated order, every field and the per-step voltages, bit for bit
        AC.same_snapshots(AC.stated_run(name, seed=int(g["seed"])), snaps, name)


def test_input_monitor_and_leftover_s():
    """Monitor(input, ["s"]) of an analog run is float32 and a copy; an unreset float `s` promotes the next byte run (its monitor then
    holds 0.0 / 1.0 as float32); a byte `s` in front of a float run is read by value; after a reset none of it is observable."""
    ns = _ns()
    name = "left_float_byte"
    net = AC.build(ns, name).to(DEV)
    inp, shape, T, B, _ = AC.case_meta(name)
    mon = ns.Monitor(net.layers[inp], ["s"], time=None)
    net.add_monitor(mon, name="Xs")
    xf, xb = AC.case_runs(name, 0)
    xfd = _dev(xf)
    net.run({inp: xfd}, time=T)
    rec = mon.get("s")
    assert rec.dtype == torch.float32 and _same(rec.reshape(T, B, -1), xf) and rec.data_ptr() != xfd.data_ptr()
    assert net.layers[inp].s.dtype == torch.float32 and net.layers[inp].s.data_ptr() == xfd[T - 1].data_ptr()
    net.run({inp: _dev(xb)}, time=T)                         # not reset: promoted
    rec = mon.get("s")
    assert net.last_plan == "generic" and rec.dtype == torch.float32 and _same(rec.reshape(T, B, -1), xb.astype(np.float32))
    net.reset_state_variables()
    net.run({inp: _dev(xb)}, time=T)                         # reset: a byte run like any other
    rec = mon.get("s")
    assert rec.dtype in (torch.uint8, torch.bool) and np.array_equal(rec.cpu().numpy().reshape(T, B, -1) != 0, xb != 0)
    summed = net.layers["Y"].summed.clone()
    net.reset_state_variables()
    del net.monitors["Xs"]
    fresh = AC.build(ns, name).to(DEV)
    fresh.run({inp: _dev(xb)}, time=T)
    assert torch.equal(fresh.layers["Y"].summed.view(torch.int32), summed.view(torch.int32))


def _zero_one_runs(name, as_float):
    def runs(n, r):
        inp, shape, T, B, _ = AC.case_meta(n)
        x = (np.random.default_rng(40 + r).random((T, B, *shape)) < 0.35).astype(np.uint8)
        return [x.astype(np.float32) if as_float else x]
    return runs


@pytest.mark.parametrize("name", ["mlp_fl_b3", "cnn_fl", "tr_pv"])
def test_whole_run_zero_one_invariance(name, monkeypatch):
    """A converted MLP, a converted CNN (pooled firing_rates included) and the traced graph: float32 zeros and ones give every field
    the same spikes give as uint8 -- rasters, per-step v, v, refrac_count, x, summed, firing_rates, the Input's per-step trace."""
    ns = _ns()
    snaps = {}
    for as_float in (False, True):
        monkeypatch.setattr(AC, "case_runs", _zero_one_runs(name, as_float))
        net = AC.build(ns, name).to(DEV)
        snaps[as_float] = AC.run_case(ns, net, name, device=DEV)
        assert net.last_plan == "generic" or not as_float
    assert any(k.endswith("_fr") for k in snaps[True][0]) == (name == "cnn_fl")
    assert all(int(v.sum()) > 0 for s in snaps[True] for k, v in s.items() if k.endswith("_raster"))
    AC.same_snapshots(snaps[False], snaps[True], name)


def test_masks_bias_and_norm_without_a_rule():
    """masks=, a bias and a `norm` without a rule work as on the byte path: the same run fed bytes and fed their float32 values."""
    ns = _ns()
    rng = np.random.default_rng(9)
    w, b = AC.dyadic(rng, 20, 12), AC.dyadic(rng, 12)
    mask = torch.from_numpy(rng.random((20, 12)) < 0.3)
    x = (rng.random((12, 2, 20)) < 0.4).astype(np.uint8)
    got = {}
    for as_float in (False, True):
        net = ns.Network(dt=1.0, batch_size=2)
        net.add_layer(ns.Input(n=20), name="X")
        net.add_layer(ns.SIF(n=12, thresh=1.0, reset=0.0, refrac=0, sum_input=True), name="Y")
        net.add_connection(ns.Connection(net.layers["X"], net.layers["Y"], w=torch.from_numpy(np.abs(w) + 0.125), b=torch.from_numpy(b), norm=3.0), "X", "Y")
        net.to(DEV)
        xd = _dev(x.astype(np.float32) if as_float else x)
        net.run({"X": xd}, time=12, masks={("X", "Y"): mask})
        assert net.last_plan == "generic"
        got[as_float] = (net.layers["Y"].summed.clone(), net.layers["Y"].v.clone(), net.connections[("X", "Y")].w.detach().clone())
    for a, c in zip(got[False], got[True]):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert float(got[True][0].abs().sum()) > 0 and bool((got[True][2][mask.to(DEV)] == 0).all())


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def _net(conn_of, target=None, n_in=12):
    ns = _ns()
    net = ns.Network(dt=1.0, batch_size=2)
    net.add_layer(ns.Input(n=n_in, traces=True), name="X")
    net.add_layer(target(ns) if target else ns.LIFNodes(n=6, traces=True), name="Y")
    net.add_connection(conn_of(ns, net.layers["X"], net.layers["Y"]), "X", "Y")
    return net.to(DEV)


def test_refusals_leave_the_state_unchanged():
    from bindsnet_amd.learning import PostPre, Hebbian
    from bindsnet_amd.network import nodes, topology, topology_features
    x = torch.from_numpy(AC.real_values(np.random.default_rng(1), 3 * 2, 12).reshape(3, 2, 12)).to(DEV)
    run = dict(inputs={"X": x}, time=3)
    # another connection class out of an analog Input: named, and still with the words the byte path used
    _refused(_net(lambda ns, a, b: topology.SparseConnection(a, b, w=(torch.rand(12, 6) * (torch.rand(12, 6) < 0.5)).to_sparse())), NotImplementedError,
             "SparseConnection.*uint8 or bool", **run)
    _refused(_net(lambda ns, a, b: topology.MulticompartmentConnection(a, b, device="cpu", pipeline=[topology_features.Weight("w", value=torch.rand(12, 6))])),
             NotImplementedError, "MulticompartmentConnection.*uint8 or bool", **run)
    _refused(_gather_net(lambda ns, a, b: ns.PermuteConnection(a, b, dims=(0, 3, 1, 2))), NotImplementedError, "PermuteConnection.*uint8 or bool",
             inputs={"X": torch.rand(3, 2, 2, 3, 5, device=DEV)}, time=3)
    # a learning rule on a connection out of an analog Input
    _refused(_net(lambda ns, a, b: ns.Connection(a, b, w=torch.rand(12, 6), update_rule=PostPre, nu=(1e-2, 1e-2))), NotImplementedError, "PostPre", **run)
    _refused(_net(lambda ns, a, b: ns.Connection(a, b, w=torch.rand(12, 6), update_rule=Hebbian, nu=(1e-2, 1e-2))), NotImplementedError, "Hebbian", **run)
    # a CSRM target
    _refused(_net(lambda ns, a, b: ns.Connection(a, b, w=torch.rand(12, 6)), target=lambda ns: nodes.CSRMNodes(n=6)), NotImplementedError, "CSRMNodes", **run)
    # floating dtypes other than float32
    good = _net(lambda ns, a, b: ns.Connection(a, b, w=torch.rand(12, 6)))
    for dt in (torch.float64, torch.float16, torch.bfloat16):
        _refused(good, NotImplementedError, r"\.float\(\)", inputs={"X": x.to(dt)}, time=3)
    good.run(**run)                                          # ... and the graph itself runs
    assert good.last_plan == "generic"


def test_multi_device_modes_refuse_an_analog_input():
    from bindsnet_amd import parallel
    net = _net(lambda ns, a, b: ns.Connection(a, b, w=torch.rand(12, 6)))
    x = torch.rand(3, 2, 12, device=DEV)
    v = net.layers["Y"].v.clone()
    for mode in (parallel.sharded_run, parallel.exact_run):
        with pytest.raises(NotImplementedError, match="uint8 or bool"):
            mode(net, {"X": x}, time=3)
        assert torch.equal(net.layers["Y"].v, v) and not net.layers["X"].x.any()
