"""CSRMNodes on the HOST: the host path (network/host_path.py) against every reference-generated fixture of
tests/golden/make_golden_csrm.py (cases in tests/csrm_cases.py), bit for bit, v included; the stated order of the device kernels
(csrm_cases.stated_run, plain torch, no package code) against the same fixtures -- everything discrete bit for bit, v within the
fixture's own `v_spread`; the raising calls; the `bindsnet` alias; the shapes, dtype and slot order of `s_w` and `last_spikes`."""
import json
import os

import numpy as np
import pytest
import torch

import cases
import csrm_cases as CC
from bindsnet_amd.network.nodes import CSRMNodes        # noqa: F401  (what every test of this file is about)

DISCRETE = ("raster", "theta", "last", "s_w", "xX", "xY", "w")


def _ns():
    from bindsnet_amd import learning
    from bindsnet_amd.network import Network, nodes, topology
    return CC.ns_from(nodes, topology, learning, Network)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gold(name):
    return cases.gold("csrm_" + name)


def build(name):
    """The case's network with this package's classes, at the fixture's seed."""
    return CC.build(_ns(), CC.CASES[name], int(gold(name)["seed"]), decays=decays(name))


def decays(name):
    """The `decay` / `theta_decay` buffers of the per-neuron case as the fixture's host made them (csrm_cases docstring)."""
    g = gold(name)
    return (g["decay"], g["theta_decay"]) if CC.CASES[name]["pervec"] else None


def same(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    got, ref = _bits(got).reshape(-1), _bits(ref).reshape(-1)
    assert np.array_equal(got, ref), f"{what} differs at {np.flatnonzero(got != ref)[:5]} of {got.size}"


def check_snapshots(name, snaps, against=None, v_exact=False, first=0):
    """Snapshots against the fixture (or against `against`, a list of snapshots): everything discrete bit for bit; v bit for bit
    (`v_exact`) or within the case's v_spread."""
    g = gold(name)
    for i, s in enumerate(snaps):
        r = first + i
        ref = {k: g[f"r{r}_{k}"] for k in DISCRETE + ("v",)} if against is None else dict(against[r])
        if against is None:
            ref["raster"] = cases.unpack(ref["raster"], s["raster"].shape)
        assert 0 < ref["raster"].sum() < ref["raster"].size, "vacuous"
        assert np.array_equal(s["raster"], ref["raster"]), \
            f"case {name} input {r}: raster differs ({int(s['raster'].sum())} vs {int(ref['raster'].sum())} spikes)"
        for k in DISCRETE[1:]:
            same(s[k], ref[k], f"case {name} input {r}: {k}")
        if v_exact:
            same(s["v"], ref["v"], f"case {name} input {r}: v")
        else:
            d = float(np.abs(s["v"].astype(np.float64) - ref["v"].astype(np.float64)).max())
            assert d <= float(g["v_spread"]), f"case {name} input {r}: |v - reference| = {d:.3g} > v_spread {float(g['v_spread']):.3g}"


@pytest.fixture(scope="module")
def stated():
    """The stated order of every case, computed once."""
    torch.set_num_threads(1)
    return {name: CC.stated_run(c, int(gold(name)["seed"]), record_v=True, decays=decays(name)) for name, c in CC.CASES.items()}


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_host_path_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    torch.set_num_threads(1)
    net = build(name)
    snaps = CC.run_case(net, CC.CASES[name], int(gold(name)["seed"]), Monitor)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps, v_exact=True)
    Y, g = net.layers["Y"], gold(name)
    for key in ("decay", "theta_decay", "resKernel", "refKernel"):
        same(getattr(Y, key).numpy(), g[key], f"case {name}: {key}")


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_stated_order_matches_reference_fixture(name, stated):
    g = gold(name)
    assert float(g["min_margin"]) >= CC.MARGIN_FACTOR * float(g["v_spread"])
    check_snapshots(name, stated[name])


def test_fixture_conditions_cover_the_cases():
    assert any(float(gold(n)["v_spread"]) > 0 for n in CC.CASES), "no case in which the order shows at all"
    assert {"AlphaKernel", "AlphaKernelSLAYER", "LaplacianKernel", "ExponentialKernel", "TriangularKernel"} == \
        {c["kernel"] for c in CC.CASES.values()}
    c = CC.CASES["learn100"]
    assert (c["src"], c["N"], c["T"], c["rule"], c["nu"]) == ((100,), 100, 250, "PostPre", 1e-2)


def test_split_run_equals_whole_on_the_host():
    from bindsnet_amd.network.monitors import Monitor
    name = "two_inputs"
    snaps = CC.run_case(build(name), CC.CASES[name], int(gold(name)["seed"]), Monitor, halves=True)
    check_snapshots(name, snaps, v_exact=True)


def test_clamp_unclamp_and_injected_voltage_on_the_host():
    """run(clamp=, unclamp=, injects_v=) against the stated order, which places them as network.py:398-429 does.  The case's
    v_spread is 0 at 12 neurons: torch's own order is the stated one there, so v is compared to the bit as well."""
    from bindsnet_amd.network.monitors import Monitor
    name = "two_inputs"
    c, seed = CC.CASES[name], int(gold(name)["seed"])
    clamp, unclamp = torch.zeros(c["N"], dtype=torch.bool), torch.zeros(c["N"], dtype=torch.bool)
    clamp[1] = clamp[7] = unclamp[7] = unclamp[4] = True
    inject = torch.linspace(-0.5, 0.5, c["N"])
    want = CC.stated_run(c, seed, clamp=clamp, unclamp=unclamp, inject_v=inject)
    snaps = CC.run_case(build(name), c, seed, Monitor, clamp={"Y": clamp}, unclamp={"Y": unclamp}, injects_v={"Y": inject})
    assert want[0]["raster"][:, :, 1].all() and not want[0]["raster"][:, :, 7].any()
    check_snapshots(name, snaps, against=want, v_exact=True)


RAISES = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "csrm_raises.json")))
_TYPES = {"RuntimeError": RuntimeError, "TypeError": TypeError, "Exception": Exception, "AttributeError": AttributeError}


@pytest.mark.parametrize("name", sorted(CC.RAISING))
def test_raising_calls_raise_the_reference_types(name):
    assert RAISES[name] is not None, "the reference runs this call"
    # a connection class without a working compute_window: the reference's AttributeError half-way through the step becomes a
    # NotImplementedError that names the class, before the run
    want = NotImplementedError if name == "other_connection" else _TYPES[RAISES[name]]
    with pytest.raises(want) as e:
        CC.RAISING[name](_ns())
    assert type(e.value) is want or want is Exception
    if name == "other_connection":
        assert "MeanFieldConnection" in str(e.value)


def _state(net):
    Y, conn = net.layers["Y"], net.connections[("X", "Y")]
    s_w = conn.s_w
    return [t.clone() for t in (Y.v, Y.s, Y.x, Y.theta, Y.last_spikes, conn.w.data)] + [None if s_w is None else s_w.clone()], net.batch_size


def _unchanged(net, before):
    after = _state(net)
    assert before[1] == after[1]
    for a, b in zip(before[0], after[0]):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("what", ["rectangular", "dt_half", "float_res_window", "batch_change"])
def test_run_time_refusals_leave_the_state_untouched(what):
    ns = _ns()
    if what == "batch_change":
        net = CC._small(ns)
        net.run({"X": CC._spikes(3, 1)}, time=3)
        x, time, err = CC._spikes(3, 2), 3, RuntimeError
    else:
        kw, dt, err = {"rectangular": (dict(responseKernel="RectangularKernel"), 1.0, RuntimeError),
                       "dt_half": ({}, 0.5, RuntimeError),
                       "float_res_window": (dict(res_window_size=20.5), 1.0, TypeError)}[what]
        net = CC._small(ns, dt=dt, **kw)
        x, time = CC._spikes(6, 1), 3
    before = _state(net)
    with pytest.raises(err):
        net.run({"X": x}, time=time)
    _unchanged(net, before)


def test_importable_from_both_package_names():
    import bindsnet.network.nodes as alias
    import bindsnet_amd.network.nodes as real
    assert alias.CSRMNodes is real.CSRMNodes is CSRMNodes
    from bindsnet.network.nodes import CSRMNodes as again
    assert again is CSRMNodes


def test_buffers_and_constructor_mirror_the_reference():
    import inspect
    Y = CSRMNodes(n=5)
    want = ["rest", "thresh", "tau", "reset_const", "res_window_size", "ref_window_size", "tc_decay", "decay", "theta_plus",
            "tc_theta_decay", "theta_decay", "v", "last_spikes", "theta", "resKernel", "refKernel"]
    assert [k for k, _ in Y.named_buffers() if k != "s"] == want
    params = list(inspect.signature(CSRMNodes.__init__).parameters)
    assert params[1:-1] == ["n", "shape", "traces", "traces_additive", "tc_trace", "trace_scale", "sum_input", "rest", "thresh",
                            "responseKernel", "refractoryKernel", "tau", "res_window_size", "ref_window_size", "reset_const", "tc_decay",
                            "theta_plus", "tc_theta_decay", "lbound"]


def test_window_state_shapes_dtype_and_slot_order():
    ns = _ns()
    net = ns.Network(batch_size=2)
    X, Y = ns.Input(shape=[2, 3], traces=True), ns.CSRMNodes(n=4, res_window_size=5, ref_window_size=3)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    conn = ns.Connection(X, Y, w=torch.zeros(6, 4))
    net.add_connection(conn, source="X", target="Y")
    assert conn.s_w is None and "s_w" not in dict(conn.named_buffers())
    assert Y.last_spikes.shape == (2, 3, 4) and Y.last_spikes.dtype == torch.float32 and not Y.last_spikes.any()
    assert Y.resKernel.shape == (5,) and Y.refKernel.shape == (3,)
    x = torch.zeros(4, 2, 2, 3, dtype=torch.uint8)
    x[0, 0, 0, 0] = x[1, 1, 1, 2] = 1
    net.run({"X": x}, time=4)
    # compute_window pushes the source's spikes of the PREVIOUS step: after 4 steps the window holds steps -1, 0, 1, 2 behind one
    # empty slot, oldest first
    assert conn.s_w.shape == (2, 5, 2, 3) and conn.s_w.dtype == torch.float32
    want = torch.zeros(2, 5, 2, 3)
    want[0, 2, 0, 0] = want[1, 3, 1, 2] = 1
    assert torch.equal(conn.s_w, want)
    Y.thresh.fill_(-1000.0)                       # every neuron spikes from now on
    net.run({"X": x[:2]}, time=2)
    assert torch.equal(Y.last_spikes[:, -2:], torch.ones(2, 2, 4)) and not Y.last_spikes[:, 0].any()
    net.reset_state_variables()                   # the windows survive the reset (a quirk of the reference)
    assert Y.last_spikes[:, -2:].all() and conn.s_w.any() and float(Y.v[0, 0]) == -65.0
    with pytest.raises(AttributeError):
        ns.Connection(X, ns.nodes.LIFNodes(n=4)).s_w


def test_multi_device_modes_refuse_the_layer():
    from bindsnet_amd import parallel
    net = CC._small(_ns())
    for call in (lambda: parallel.sharded_run(net, {"X": CC._spikes(3, 1)}, time=3), lambda: parallel.column_shard(net, 0, 2),
                 lambda: parallel.exact_run(net, {"X": CC._spikes(3, 1)}, time=3)):
        with pytest.raises(NotImplementedError, match="CSRMNodes"):
            call()
