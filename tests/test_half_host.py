"""float16 / bfloat16 Weight features on the HOST path (network/host_path.py: plain torch, as the reference computes them), no GPU:

  * every fixture case of tests/half_cases.py (tests/golden/make_golden_half.py: the unmodified reference at one thread) bit for bit --
    both rasters, v, refrac_count, theta, both traces, the learned value's raw 16-bit patterns and the generator's state, after each
    of 3 inputs;
  * what a half Weight refuses, by name of the dtype, at construction or before a run changes any state;
  * a float32 DiehlAndCook2015 is untouched: same descriptor route (w_dtype 0) and the values of an existing fixture."""
import os

import numpy as np
import pytest
import torch

import half_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = ("vE", "vI", "theta", "refracE", "refracI", "xX", "xE")
HALVES = (torch.float16, torch.bfloat16)


def gold(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"half_{name}.npz"))


def ns():
    from bindsnet_amd import models
    from bindsnet_amd.network import monitors
    return HC.ns_from(models, monitors)


def build(name, **over):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)       # "Provided value has data type torch.float32 but parameter w_dtype is ..."
        return HC.build(ns(), name, **over)


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} elements differ"


def check_snapshots(name, snaps, first=0, rng=True):
    g, c = gold(name), HC.CASES[name]
    for k, s in enumerate(snaps):
        r = first + k
        for key in ("sE", "sI"):
            want = np.unpackbits(g[f"r{r}_{key}"])[:s[key].size].reshape(s[key].shape)
            same(s[key], want, f"case {name} input {r}: {key} raster")
            assert int(s[key].sum()) == int(g[f"r{r}_{key}_sum"])
        for key in FLOATS:
            same(s[key], g[f"r{r}_{key}"], f"case {name} input {r}: {key}")
        same(s["value"], g[f"r{r}_value"], f"case {name} input {r}: value ({c['dtype']} bit patterns)")
        if rng:
            assert HC.sha(s["rng"]) == str(g[f"r{r}_rng_sha"]), f"case {name} input {r}: the generator's state"


@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_host_path_equals_the_reference_on_every_case(name):
    from bindsnet_amd.network.monitors import Monitor
    net = build(name)
    assert HC.value_of(net).dtype == HC.dtype_of(name)
    assert HC.sha(HC.bits16(HC.value_of(net))) == str(gold(name)["value0_sha"])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        snaps = HC.run_case(net, name, Monitor)
    finally:
        torch.set_num_threads(threads)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps)


def _layers():
    from bindsnet_amd.network.nodes import Input, LIFNodes
    return Input(n=6, traces=True), LIFNodes(n=5, traces=True)


@pytest.mark.parametrize("dtype", HALVES)
def test_constructor_refusals_name_the_dtype(dtype):
    from bindsnet_amd.learning import MCC_learning
    from bindsnet_amd.network import topology
    from bindsnet_amd.network.topology_features import Weight
    w = torch.rand(6, 5).to(dtype)
    for rule in (MCC_learning.MSTDP, MCC_learning.MSTDPET):
        X, Y = _layers()
        with pytest.raises(NotImplementedError, match=str(dtype)):
            topology.MulticompartmentConnection(X, Y, device="cpu", pipeline=[Weight("w", w.clone(), value_dtype=dtype, learning_rule=rule,
                                                                                     nu=(1e-2, 1e-2), range=[0.0, 1.0])])
    with pytest.raises(NotImplementedError, match=str(dtype)):
        Weight("w", w.clone(), value_dtype=dtype, norm=torch.ones(5))
    # every connection class with a `w` keeps its float32-only refusal
    X, Y = _layers()
    for make in (lambda: topology.Connection(X, Y, w_dtype=dtype), lambda: topology.SparseConnection(X, Y, w_dtype=dtype, sparsity=0.5),
                 lambda: topology.MeanFieldConnection(X, Y, w_dtype=dtype)):
        with pytest.raises(NotImplementedError, match="float32 only"):
            make()
    # PostPre and NoOp are accepted
    X, Y = _layers()
    topology.MulticompartmentConnection(X, Y, device="cpu", pipeline=[Weight("w", w.clone(), value_dtype=dtype, learning_rule=MCC_learning.PostPre,
                                                                             nu=(1e-2, 1e-2), range=[0.0, 1.0], norm=2.0)])


@pytest.mark.parametrize("dtype", HALVES)
def test_run_refusals_come_before_any_state_changes(dtype):
    from bindsnet_amd import parallel
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.monitors import Monitor
    from bindsnet_amd.network.topology import MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Weight
    X, Y = _layers()
    feat = Weight("w", torch.rand(6, 5).to(dtype), value_dtype=dtype)
    conn = MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat])
    net = Network()
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(conn, "X", "Y")
    x = torch.ones(3, 2, 6, dtype=torch.uint8)
    before = (Y.v.clone(), feat.value.clone(), net.batch_size)
    net.add_monitor(Monitor(feat, ["value"], time=3), "value")
    with pytest.raises(NotImplementedError, match=str(dtype)):
        net.run({"X": x}, time=3)
    del net.monitors["value"]
    for mode in (lambda: parallel.sharded_run(net, {"X": x}, 3), lambda: parallel.column_shard(net, 0, 2), lambda: parallel.exact_run(net, {"X": x}, 3)):
        with pytest.raises(NotImplementedError, match=str(dtype)):
            mode()
    assert torch.equal(Y.v, before[0]) and torch.equal(feat.value, before[1]) and net.batch_size == before[2]
    net.run({"X": x}, time=3)                              # ... and without them the host path runs it
    assert net.last_plan == "host-torch" and feat.value.dtype == dtype


def test_float64_stays_refused_on_the_device_route():
    """_describe is what a device run asks first: float64 is still turned away there, float16 / bfloat16 set w_dtype."""
    from bindsnet_amd import _lib
    from bindsnet_amd.network.topology import MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Weight

    class Dev:                                             # (no GPU here: a value that is where the run wants it)
        pass
    for dtype, code in ((torch.float32, 0), (torch.float16, 1), (torch.bfloat16, 2), (torch.float64, None)):
        X, Y = _layers()
        conn = MulticompartmentConnection(X, Y, device="cpu", pipeline=[Weight("w", torch.rand(6, 5).to(dtype), value_dtype=dtype, norm=1.0)])
        d = _lib.ConnDesc()
        scratch = lambda key, shape, dt, dev: torch.empty(shape, dtype=dt)      # noqa: E731
        if code is None:
            with pytest.raises(NotImplementedError, match="float64"):
                conn._describe(d, 1, torch.device("cpu"), scratch)
        else:
            conn._describe(d, 1, torch.device("cpu"), scratch)
            assert d.w_dtype == code and d.has_norm == 1 and d.pipe_n == 0


def test_float32_model_is_untouched():
    """The default DiehlAndCook2015 still builds float32 values that describe themselves with w_dtype 0, and the host path still gives
    the float32 fixture's values (the loader and the check of tests/test_host_path.py)."""
    from bindsnet_amd import _lib
    from bindsnet_amd.models import DiehlAndCook2015
    torch.manual_seed(0)
    net = DiehlAndCook2015(n_inpt=784, n_neurons=40)
    for conn in net.connections.values():
        assert conn.pipeline[0].value.dtype == torch.float32 and conn._half_dtype() is None and conn._run_refusal(None, True) is None
        d = _lib.ConnDesc()
        conn._describe(d, 1, torch.device("cpu"), lambda key, shape, dt, dev: torch.empty(shape, dtype=dt))
        assert d.w_dtype == 0
    import test_host_path as THP
    THP.test_dc2015_on_the_host_matches_reference("run_dc_n100_b3")
