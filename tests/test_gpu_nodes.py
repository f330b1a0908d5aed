"""McCullochPitts / IFNodes / BoostedLIFNodes / CurrentLIFNodes / IzhikevichNodes on the MI355X (csrc/snn_nodes.hip), bit for bit.

  * every reference-generated fixture case of tests/node_cases.py on the device, generic plan; two half runs equal one whole run;
    the `s` / `v` monitors are the fixture's per-step record;
  * against the host path (network/host_path.py, itself pinned to the same fixtures by tests/test_nodes_host.py): clamp / unclamp /
    injects_v, each layer's standalone forward(), a new layer where a fused plan would otherwise match, kernel sizes that straddle
    the launch limits, and the breakout-shaped graph (dense Connection + MSTDP)."""
import numpy as np
import pytest
import torch

import node_cases as NC
from test_nodes_host import _bits, _ns, build, check_snapshots, gold

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def few_host_threads():
    """The checker of most tests is the plain-PyTorch host path: at the GPU box's default thread count every small operator of it takes
    milliseconds."""
    n = torch.get_num_threads()
    torch.set_num_threads(min(4, n))
    yield
    torch.set_num_threads(n)


def _classes():
    from bindsnet_amd.network import nodes
    return {"mcp": nodes.McCullochPitts, "if": nodes.IFNodes, "boosted": nodes.BoostedLIFNodes, "clif": nodes.CurrentLIFNodes,
            "izh": nodes.IzhikevichNodes}


def _state(layer):
    out = {k: getattr(layer, k).detach().cpu().numpy().astype(np.float32).copy() for k in NC.STATE
           if isinstance(getattr(layer, k, None), torch.Tensor)}
    out["s"] = layer.s.detach().cpu().numpy().astype(np.uint8).copy()
    return out


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in got:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        a, b = (a, b) if a.dtype == np.uint8 else (_bits(a), _bits(b))
        bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} of {a.size} elements (first {bad[:5]})"


# ------------------------------------------------------------------ reference fixtures
@pytest.mark.parametrize("name", sorted(NC.CASES))
def test_device_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    net = build(name).to(DEV)
    snaps = NC.run_case(net, name, Monitor, device=DEV)
    assert net.last_plan == "generic"
    check_snapshots(name, snaps)               # raster and v record come from the device monitors


@pytest.mark.parametrize("name", ["mcp_b4", "if_b4", "boosted_mcc", "clif_b4", "clif_mcc", "izh_mix_b4", "izh_e0_b4", "izh_mcc", "if_b4_dt01", "clif_b4_dt2",
                                  "izh_e0_b1_dt03", "if_mcc_dt03"])
def test_two_half_runs_equal_one_whole_run(name):
    from bindsnet_amd.network.monitors import Monitor
    net = build(name).to(DEV)
    snaps = NC.run_case(net, name, Monitor, device=DEV, halves=True)
    assert net.last_plan == "generic"
    check_snapshots(name, snaps)


# ------------------------------------------------------------------ against the host path
def _layer(kind, n, B, dev, seed=0, **kw):
    torch.manual_seed(seed)
    layer = _classes()[kind](n=n, traces=True, **kw)
    layer.compute_decays(1.0)
    layer.set_batch_size(B)
    layer.to(dev)
    layer.set_batch_size(B)
    return layer


CURRENT = {"mcp": (-0.5, 1.5), "if": (-2.0, 5.0), "boosted": (-1.0, 5.0), "clif": (-0.5, 2.0), "izh": (0.0, 12.0)}
EXTRA = {"mcp": {}, "if": dict(lbound=-66.0, refrac=3), "boosted": dict(refrac=2), "clif": dict(lbound=-65.25, refrac=3),
         "izh": dict(excitatory=0.8, lbound=-70.0)}


def _current(kind, T, B, n, seed):
    lo, hi = CURRENT[kind]
    return (lo + (hi - lo) * np.random.default_rng(seed).random((T, B, n), dtype=np.float32)).astype(np.float32)


def _hand_step(kind, n, B, T, seed=0, **kw):
    """T standalone forward() calls on the host and on the device; returns the per-step spike record of the host (for vacuity
    checks) after comparing every step's spikes and the final state."""
    cur = _current(kind, T, B, n, seed + 50)
    rec = {}
    for dev in ("cpu", DEV):
        layer = _layer(kind, n, B, dev, seed, **{**EXTRA[kind], **kw})
        ss = []
        for t in range(T):
            x = torch.from_numpy(cur[t].copy()).to(dev)
            layer.forward(x)
            ss.append(layer.s.cpu().numpy().astype(np.uint8).copy())
        rec[dev] = (np.stack(ss), _state(layer))
    bad = np.flatnonzero((rec["cpu"][0] != rec[DEV][0]).reshape(T, -1).any(1))
    assert bad.size == 0, f"{kind} n={n} B={B}: spikes differ first at step {bad[:1]}"
    _same(rec[DEV][1], rec["cpu"][1], f"{kind} n={n} B={B} after {T} steps")
    return rec["cpu"][0]


@pytest.mark.parametrize("kind", NC.KINDS)
def test_standalone_forward_equals_the_host_step(kind):
    spikes = _hand_step(kind, 70, 3, 25)
    assert 0 < spikes.sum() < spikes.size, "vacuous"


@pytest.mark.parametrize("kind", ["mcp", "if", "boosted", "clif"])
@pytest.mark.parametrize("B,n", [(3, 101), (1, 255), (5, 257), (33, 32768)])
def test_pointwise_kernels_across_their_launch_limits(kind, B, n):
    """B*n not a multiple of 256, below / above one block, and (33 x 32768 = 1 081 344 > 4096 blocks x 256) past the grid cap, where
    the grid-stride loop takes a second pass."""
    spikes = _hand_step(kind, n, B, 6 if n > 1000 else 12)
    assert spikes.sum() > 0


@pytest.mark.parametrize("n", [1, 7, 63, 64, 65, 100, 130, 1000, 1024])
def test_izhikevich_sizes_that_are_not_whole_waves(n):
    _hand_step("izh", n, 3, 12)


@pytest.mark.parametrize("k", [0, 1, 7, 8, 9, 150])
def test_izhikevich_lateral_sum_at_chosen_spike_counts(k):
    """Exactly k entry spikes (0, 1, 7, 8, 9 and n: both branches of the summation order and their edges), one step."""
    n, B = 150, 4
    rng = np.random.default_rng(k)
    s0 = np.zeros((B, n), bool)
    for b in range(B):
        s0[b, rng.choice(n, k, replace=False)] = True
    cur = _current("izh", 1, B, n, 9)[0]
    out = {}
    for dev in ("cpu", DEV):
        layer = _layer("izh", n, B, dev, 1, excitatory=0.8)
        layer.s = torch.from_numpy(s0.copy()).to(dev)
        x = torch.from_numpy(cur.copy()).to(dev)
        layer.forward(x)
        out[dev] = dict(_state(layer), current=x.cpu().numpy())
    if k:                                      # (without a spike the reference adds nothing; the kernel adds +0)
        assert np.abs(out["cpu"]["current"] - cur).max() > 0
    _same(out[DEV], out["cpu"], f"k = {k}")


def _run_both(make, inputs, T, **kwargs):
    """The same network on the host and on the device; returns {dev: (network, monitors' records)}."""
    from bindsnet_amd.network.monitors import Monitor
    out = {}
    for dev in ("cpu", DEV):
        net = make()
        mons = {}
        for lname, layer in net.layers.items():
            if hasattr(layer, "v"):
                mons[lname] = Monitor(layer, ["s", "v"], time=T)
                net.add_monitor(mons[lname], lname)
        net.to(dev)
        kw = {k: ({n: (torch.as_tensor(t).to(dev)) for n, t in v.items()} if isinstance(v, dict) else v) for k, v in kwargs.items()}
        net.run({k: torch.from_numpy(v.copy()).to(dev) for k, v in inputs.items()}, time=T, **kw)
        rec = {l: (m.get("s").cpu().numpy().astype(np.uint8), m.get("v").cpu().numpy()) for l, m in mons.items()}
        out[dev] = (net, rec)
    return out


def _compare_runs(out, what, dense_family=False):
    """dense_family=False: rasters, voltage records, final state and weights bit for bit.
    dense_family=True: the bar of the dense family against a host run (tests/test_gpu_baseline_configs.py
    test_dense_family_full_size_matches_reference, tests/test_gpu_network.py): the host's `s @ w` is an MKL sgemm whose summation order is
    not the device's ascending one, so rasters identical, weights within 1e-5, and everything that is a function of the rasters alone
    (traces, refractory counters, the rule's P+ / P- / eligibility) bit for bit; the voltages are printed, not compared."""
    (hn, hrec), (dn, drec) = out["cpu"], out[DEV]
    assert hn.last_plan == "host-torch" and dn.last_plan == "generic", (hn.last_plan, dn.last_plan)
    for l in hrec:
        dv = np.abs(hrec[l][1].astype(np.float64) - drec[l][1].astype(np.float64)).reshape(hrec[l][1].shape[0], -1).max(1)
        first = np.flatnonzero(dv > 0)
        print(f"{what}: layer {l}: host spikes {int(hrec[l][0].sum())}, device spikes {int(drec[l][0].sum())}, spike mismatches "
              f"{int((hrec[l][0] != drec[l][0]).sum())}, v elements that differ {int((_bits(hrec[l][1]) != _bits(drec[l][1])).sum())} of "
              f"{hrec[l][1].size}, max |dv| {float(dv.max()):.3g}" +
              (f", first at step {int(first[0])} with max |dv| {float(dv[first[0]]):.3g}" if first.size else ""))
    for key, conn in hn.connections.items():
        if hasattr(conn, "w"):
            wh, wd = conn.w.detach().cpu().numpy(), dn.connections[key].w.detach().cpu().numpy()
            print(f"{what}: connection {key}: w elements that differ {int((_bits(wh) != _bits(wd)).sum())} of {wh.size}, max |dw| "
                  f"{float(np.abs(wh - wd).max()):.3g}")
    for l in hrec:
        np.testing.assert_array_equal(drec[l][0], hrec[l][0], err_msg=f"{what}: raster of {l}")
    if dense_family:
        for l in hn.layers:
            got, want = _state(dn.layers[l]), _state(hn.layers[l])
            keep = [k for k in want if k in ("s", "x", "refrac_count")]
            _same({k: got[k] for k in keep}, {k: want[k] for k in keep}, f"{what}: raster-determined state of {l}")
        for key, conn in hn.connections.items():
            wh, wd = conn.w.detach().cpu().numpy(), dn.connections[key].w.detach().cpu().numpy()
            np.testing.assert_allclose(wd, wh, rtol=0, atol=1e-5, err_msg=f"{what}: weights of {key}")
            hr, dr = conn.update_rule, dn.connections[key].update_rule
            _same({k: getattr(dr, k).detach().cpu().numpy() for k in ("p_plus", "p_minus", "eligibility")},
                  {k: getattr(hr, k).detach().cpu().numpy() for k in ("p_plus", "p_minus", "eligibility")}, f"{what}: rule state of {key}")
        return
    for l in hrec:
        np.testing.assert_array_equal(_bits(drec[l][1]), _bits(hrec[l][1]), err_msg=f"{what}: v record of {l}")
        _same(_state(dn.layers[l]), _state(hn.layers[l]), f"{what}: final state of {l}")
    for key, conn in hn.connections.items():
        if hasattr(conn, "w"):
            np.testing.assert_array_equal(_bits(dn.connections[key].w.detach().cpu().numpy()), _bits(conn.w.detach().cpu().numpy()),
                                          err_msg=f"{what}: weights of {key}")


@pytest.mark.parametrize("kind", NC.KINDS)
def test_clamp_unclamp_and_inject_v_equal_the_host_path(kind):
    from bindsnet_amd.network import Network
    n, B, T = 60, 3, 20
    rng = np.random.default_rng(5)
    clamp = torch.from_numpy(rng.random((T, n)) < 0.05)
    unclamp = torch.from_numpy(rng.random(n) < 0.2)
    inject = torch.from_numpy((rng.random((T, n), dtype=np.float32) * 2 - 0.5).astype(np.float32))

    def make():
        net = Network(dt=1.0)
        torch.manual_seed(2)
        net.add_layer(_classes()[kind](n=n, traces=True, **EXTRA[kind]), "Y")
        return net

    out = _run_both(make, {"Y": _current(kind, T, B, n, 3)}, T, clamp={"Y": clamp}, unclamp={"Y": unclamp}, injects_v={"Y": inject})
    assert out["cpu"][1]["Y"][0].sum() > 0
    _compare_runs(out, f"{kind} with clamp / unclamp / injects_v")


def test_new_layer_where_a_fused_plan_would_match_runs_generic():
    """Input -> Connection -> LIFNodes is the two-layer fused plan's graph; with IFNodes in the LIF layer's place the graph takes
    the generic plan and equals the host path (weights on a 1/4 grid: the currents are exact in any summation order)."""
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import IFNodes, Input, LIFNodes
    from bindsnet_amd.network.topology import Connection
    n_in, n, B, T = 64, 32, 2, 40
    w = (np.random.default_rng(0).integers(0, 8, (n_in, n)) * 0.25).astype(np.float32)
    x = (np.random.default_rng(1).random((T, B, n_in)) < 0.1).astype(np.uint8)

    def make(cls=IFNodes):
        net = Network(dt=1.0)
        net.add_layer(Input(n=n_in, traces=True), "X")
        net.add_layer(cls(n=n, traces=True), "Y")
        net.add_connection(Connection(net.layers["X"], net.layers["Y"], w=torch.from_numpy(w.copy())), "X", "Y")
        return net

    out = _run_both(make, {"X": x}, T)
    assert out["cpu"][1]["Y"][0].sum() > 0
    _compare_runs(out, "Input -> Connection -> IFNodes")
    lif = make(LIFNodes).to(DEV)
    lif.run({"X": torch.from_numpy(x).to(DEV)}, time=T)
    assert lif.last_plan != "generic", "the LIF twin of the graph is what a fused plan matches"


def test_izhikevich_above_the_supported_size_raises():
    from bindsnet_amd import _lib
    from bindsnet_amd.network import Network
    n = _lib.IZH_MAX_N + 1
    torch.manual_seed(0)
    net = Network(dt=1.0)
    net.add_layer(_classes()["izh"](n=n), "Y")
    net.to(DEV)
    with pytest.raises(NotImplementedError, match=str(_lib.IZH_MAX_N)):
        net.run({"Y": torch.zeros(2, 1, n, device=DEV)}, time=2)
    layer = _layer("izh", n, 1, DEV)
    with pytest.raises(NotImplementedError, match=str(_lib.IZH_MAX_N)):
        layer.forward(torch.zeros(1, n, device=DEV))


def test_monitoring_another_state_variable_raises():
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.monitors import Monitor
    torch.manual_seed(0)
    net = Network(dt=1.0)
    net.add_layer(_classes()["izh"](n=10), "Y")
    net.add_monitor(Monitor(net.layers["Y"], ["u"], time=2), "u")
    net.to(DEV)
    with pytest.raises(NotImplementedError, match="'u'"):
        net.run({"Y": torch.zeros(2, 1, 10, device=DEV)}, time=2)


def test_lateral_matrix_changes_are_seen():
    """The transposed device copy of S follows an in-place change and a replacement of S."""
    n, B = 40, 2
    cur = _current("izh", 1, B, n, 4)[0]
    s0 = np.random.default_rng(0).random((B, n)) < 0.3

    def step(layer, dev):
        layer.reset_state_variables()
        layer.s = torch.from_numpy(s0.copy()).to(dev)
        layer.forward(torch.from_numpy(cur.copy()).to(dev))
        return _state(layer)

    host, dev = _layer("izh", n, B, "cpu", 3), _layer("izh", n, B, DEV, 3)
    _same(step(dev, DEV), step(host, "cpu"), "as constructed")
    for l in (host, dev):
        l.S.mul_(-2.0)
    _same(step(dev, DEV), step(host, "cpu"), "after S.mul_()")
    new = torch.from_numpy(np.random.default_rng(9).random((n, n), dtype=np.float32))
    host.S, dev.S = new.clone(), new.clone().to(DEV)
    _same(step(dev, DEV), step(host, "cpu"), "after S was replaced")


@pytest.mark.parametrize("B", [1, 16])
def test_breakout_shaped_graph_equals_the_host_path(B):
    """Input 6400 -> Connection (MSTDP) -> IzhikevichNodes 100 -> Connection (MSTDP) -> IzhikevichNodes 4, reward 1.0, Bernoulli input:
    device against the host path with the criterion of the existing dense-family device-versus-host tests (DESIGN.md section 2;
    tests/test_gpu_baseline_configs.py test_dense_family_full_size_matches_reference, whose cfg5 is this graph's first connection --
    Input 6400 -> Connection (MSTDP), B = 16 -- and tests/test_gpu_network.py): rasters identical, weights within 1e-5, raster-determined
    state and the rule's state bit for bit.  The host's `s @ w` goes through MKL sgemm, whose summation order at 6400 sources is not
    the device's documented ascending one, so the voltages between two spikes are not part of that criterion; they are printed (run with
    -s).  Measured once on an MI355X box with the voltages compared bit for bit as well: B = 1 equal in every bit; B = 16 rasters (3289 and
    90 spikes) and both weight matrices equal in every bit, 23075 of 64000 recorded voltages of the hidden layer different (largest 8.15,
    on the upstroke of a spike, where the Izhikevich map multiplies a difference by about ten per step), none in the output layer.
    test_breakout_shaped_graph_with_order_free_currents_is_bit_exact holds the voltages of the same graph to every bit."""
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network, nodes, topology
    T = 40
    out = _run_both(lambda: NC.breakout_graph(nodes, topology, learning, Network, "izh"), {"X": NC.breakout_input(T, B)}, T, reward=1.0)
    assert out["cpu"][1]["M"][0].sum() > 0 and out["cpu"][1]["O"][0].sum() > 0
    _compare_runs(out, f"breakout graph, B = {B}", dense_family=True)


@pytest.mark.parametrize("B", [1, 16])
def test_breakout_shaped_graph_with_order_free_currents_is_bit_exact(B):
    """The same graph and input with the weights on a 1/128 grid and no rule (node_cases.breakout_graph(fixed_grid=True)): every dense
    current is exact whatever the summation order, so what is left is the node kernels at this shape -- rasters, every recorded
    voltage, v / u / x of both Izhikevich layers bit for bit against the host path."""
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network, nodes, topology
    T = 40
    out = _run_both(lambda: NC.breakout_graph(nodes, topology, learning, Network, "izh", fixed_grid=True), {"X": NC.breakout_input(T, B)}, T)
    assert out["cpu"][1]["M"][0].sum() > 0 and out["cpu"][1]["O"][0].sum() > 0
    _compare_runs(out, f"breakout graph on a weight grid, B = {B}")
