"""SRM0Nodes and Rmax on the HOST: the uniform-draw rule the device kernel is built on, pinned against torch.rand_like itself; the
host path (network/host_path.py) against every reference-generated fixture of tests/golden/make_golden_srm0.py (cases in
tests/srm0_cases.py), bit for bit, s_prob and the generator state included; split runs; the raising paths; the `bindsnet` alias."""
import numpy as np
import pytest
import torch

import cases
import srm0_cases as SC
from bindsnet_amd.learning import Rmax                  # noqa: F401  (what every test of this file is about)
from bindsnet_amd.network.nodes import SRM0Nodes        # noqa: F401


def _ns():
    from bindsnet_amd import learning
    from bindsnet_amd.network import Network, nodes, topology, topology_features
    return SC.ns_from(nodes, topology, topology_features, learning, Network)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gold(name):
    return cases.gold("srm0_" + name)


def build(name):
    """The case's network with this package's classes; a per-neuron `decay` buffer comes from the fixture (srm0_cases.build)."""
    g = gold(name)
    decay = {L: g[f"{L}_decay"] for L in SC.srm0_layers(name)} if SC.CASES[name].get("pervec") else None
    return SC.build(_ns(), name, decay)


def same(got, ref, what):
    got, ref = _bits(got).reshape(-1), _bits(ref).reshape(-1)
    assert got.shape == ref.shape, what
    assert np.array_equal(got, ref), f"{what} differs at {np.flatnonzero(got != ref)[:5]} of {got.size}"


def check_snapshots(name, snaps, first=0, tol=None):
    """Every snapshot against the fixture.  tol None: everything bit for bit (the host path).  tol = dict(p=, v=, e=, w=): the device
    criteria -- rasters, refrac_count, traces and the generator state still exact; v, s_prob, eligibility_trace and w within the
    given absolute bounds (0 / absent: exact)."""
    g = gold(name)
    tol = tol or {}

    def close(got, ref, key, what):
        if not tol.get(key):
            return same(got, ref, what)
        d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max()
        assert d <= tol[key], f"{what}: largest difference {d:.3g} > {tol[key]:.3g}"

    for i, s in enumerate(snaps):
        r = first + i
        assert np.array_equal(s["rng0"], g[f"r{r}_rng0"]), f"case {name} input {r}: the generator stood elsewhere before the input"
        for L in SC.srm0_layers(name):
            want = cases.unpack(g[f"r{r}_{L}_raster"], s[L + "_raster"].shape)
            assert 0 < want.sum() < want.size
            assert np.array_equal(s[L + "_raster"], want), \
                f"case {name} input {r}: {L} raster differs ({int(s[L + '_raster'].sum())} vs {int(want.sum())} spikes)"
            close(s[L + "_vrec"], g[f"r{r}_{L}_vrec"], "v", f"case {name} input {r}: per-step v of {L}")
            if L + "_prec" in s:
                close(s[L + "_prec"], g[f"r{r}_{L}_prec"], "p", f"case {name} input {r}: per-step s_prob of {L}")
            close(s[L + "_v"], g[f"r{r}_{L}_v"], "v", f"case {name} input {r}: final v of {L}")
            close(s[L + "_sprob"], g[f"r{r}_{L}_sprob"], "p", f"case {name} input {r}: final s_prob of {L}")
            same(s[L + "_rc"], g[f"r{r}_{L}_rc"], f"case {name} input {r}: refrac_count of {L}")
            same(s[L + "_x"], g[f"r{r}_{L}_x"], f"case {name} input {r}: trace of {L}")
        if "xX" in s:
            same(s["xX"], g[f"r{r}_xX"], f"case {name} input {r}: Input trace")
            close(s["w"], g[f"r{r}_w"], "w", f"case {name} input {r}: weights")
        if "e" in s:
            close(s["e"], g[f"r{r}_e"], "e", f"case {name} input {r}: eligibility_trace")
        assert np.array_equal(s["rng1"], g[f"r{r}_rng1"]), f"case {name} input {r}: the generator stands elsewhere after the input"


# ---- the draw -----------------------------------------------------------------------------------------------------------------------
def _mt_next_block(mt):
    """The next 624 raw words of mt19937 after the block `mt` (uint32 [624])."""
    mt = mt.astype(np.uint64)
    out = np.zeros(624, np.uint64)

    def mix(a, b):
        y = (a & 0x80000000) | (b & 0x7FFFFFFF)
        return (y >> 1) ^ (0x9908B0DF if y & 1 else 0)

    for i in range(624):
        nxt = mt[i + 1] if i < 623 else out[0]
        far = mt[i + 397] if i + 397 < 624 else out[i - 227]
        out[i] = far ^ np.uint64(mix(int(mt[i]), int(nxt)))
    return out.astype(np.uint32)


def _temper(y):
    y = y.astype(np.uint32)
    y ^= y >> 11
    y ^= (y << 7) & np.uint32(0x9D2C5680)
    y ^= (y << 15) & np.uint32(0xEFC60000)
    y ^= y >> 18
    return y


def uniform_from_state(img, count):
    """The draw rule of snn_srm0_step on a decoded generator image (rng.torch_state_to_words): `count` uniforms, one 32-bit output
    each, u = (r & 0xFFFFFF) * 2^-24; returns them and the image afterwards."""
    img = img.copy()
    mt, pos = img[:624].view(np.uint32).copy(), int(img[624])
    out = np.zeros(count, np.float32)
    k = 0
    while k < count:
        if pos >= 624:
            mt, pos = _mt_next_block(mt), 0
        take = min(624 - pos, count - k)
        out[k:k + take] = (_temper(mt[pos:pos + take]) & np.uint32(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)
        pos += take
        k += take
    img[:624] = mt.view(np.int32)
    img[624] = pos
    return out, img


@pytest.mark.parametrize("warm", [0, 300, 623, 624])
@pytest.mark.parametrize("shape", [(1, 5), (3, 101), (1, 623), (1, 624), (2, 313), (5, 257)])
def test_uniform_draw_rule_equals_torch_rand_like(warm, shape):
    """One 32-bit mt19937 output per element, row-major, u = (r & 0xFFFFFF) * 2^-24 -- from block position "twist first" (a fresh
    seed, and 624 draws later), mid-block and 623; element counts below, at and above a block."""
    from bindsnet_amd import rng
    torch.manual_seed(17 + warm)
    if warm:
        torch.rand(warm)
    st = torch.get_rng_state()
    img = rng.torch_state_to_words(st)
    assert int(img[624]) == (624 if warm in (0, 624) else warm)
    want = torch.rand_like(torch.empty(*shape)).numpy()
    after = torch.get_rng_state()
    got, img2 = uniform_from_state(img, want.size)
    assert np.array_equal(_bits(got), _bits(want).reshape(-1))
    torch.set_rng_state(rng.words_to_torch_state(img2, st))
    a = torch.rand(700)
    torch.set_rng_state(after)
    assert torch.equal(a, torch.rand(700)), "the walked state is not where torch.rand_like leaves the generator"


def test_fixture_draws_follow_the_rule():
    """The draws the generator script recovered by replay are this rule applied to the fixture's entry state (layer order within a
    step), and the exit state is the walked one."""
    from bindsnet_amd import rng
    for name in ("d_b5n257_w623", "two"):
        g = gold(name)
        c = SC.CASES[name]
        img = rng.torch_state_to_words(torch.from_numpy(g["r0_rng0"]))
        for t in range(c["T"]):
            for L in SC.srm0_layers(name):
                want = g[f"r0_{L}_u"][t].reshape(-1)
                got, img = uniform_from_state(img, want.size)
                assert np.array_equal(_bits(got), _bits(want)), (name, t, L)
        back = rng.words_to_torch_state(img, torch.from_numpy(g["r0_rng0"]))
        assert np.array_equal(rng.torch_state_to_words(back), rng.torch_state_to_words(torch.from_numpy(g["r0_rng1"])))


# ---- the host path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_host_path_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        net = build(name)
        snaps = SC.run_case(net, name, Monitor, mode="steps")
    finally:
        torch.set_num_threads(n)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps)
    assert float(gold(name)["min_margin"]) >= SC.MARGIN[bool(SC.CASES[name].get("rule"))]


@pytest.mark.parametrize("name", ["d_b2n313_w5", "two", "mcc", "rmax_decay", "rmax_local"])
@pytest.mark.parametrize("mode", ["whole", "halves"])
def test_split_runs_equal_one_run(name, mode):
    from bindsnet_amd.network.monitors import Monitor
    check_snapshots(name, SC.run_case(build(name), name, Monitor, mode=mode))


def test_compute_decays_is_the_reference_expression():
    """exp(-dt / tc) by torch.exp, as the reference computes it: equal to the recorded buffers up to the last bit of a 1-ulp function
    (bit for bit on the CPU kind the fixtures were made on)."""
    for name in ("pervec", "dt05", "two"):
        g = gold(name)
        net = SC.build(_ns(), name)
        for L in SC.srm0_layers(name):
            for k in ("decay", "trace_decay"):
                got, ref = getattr(net.layers[L], k).numpy().astype(np.float32), g[f"{L}_{k}"]
                assert got.shape == ref.shape and np.abs(_bits(got).astype(np.int64) - _bits(ref).astype(np.int64)).max() <= 1, (name, L, k)


def test_standalone_forward_equals_a_run_step():
    from bindsnet_amd.network.monitors import Monitor
    name = "lbound"
    c = SC.CASES[name]
    snaps = SC.run_case(build(name), name, Monitor, count=1)
    Y = build(name).layers["Y"]
    Y.set_batch_size(c["B"])
    torch.set_rng_state(torch.from_numpy(snaps[0]["rng0"]))
    cur = torch.from_numpy(SC.inputs(name, 0)["Y"].copy())
    for t in range(c["T"]):
        Y.forward(cur[t])
        assert np.array_equal(Y.s.numpy().astype(np.uint8), snaps[0]["Y_raster"][t]), t
    same(Y.v.numpy(), snaps[0]["Y_v"], "final v")
    same(Y.s_prob.numpy(), snaps[0]["Y_sprob"], "final s_prob")
    assert tuple(Y.rho.shape) == tuple(Y.v.shape)
    assert torch.equal(torch.get_rng_state(), torch.from_numpy(snaps[0]["rng1"]))


# ---- construction and the raising paths ------------------------------------------------------------------------------------------------
def test_classes_import_from_both_names():
    from bindsnet.learning import Rmax
    from bindsnet.network.nodes import SRM0Nodes
    from bindsnet_amd.learning import Rmax as Rmax2
    from bindsnet_amd.network import nodes
    assert SRM0Nodes is nodes.SRM0Nodes and Rmax is Rmax2
    Y = SRM0Nodes(n=3)
    assert [k for k, _ in Y.named_buffers()] == ["s", "rest", "reset", "thresh", "refrac", "tc_decay", "decay", "eps_0", "rho_0", "d_thresh",
                                                 "v", "refrac_count"]
    assert float(Y.thresh) == -50.0 and float(Y.rest) == -70.0 and float(Y.tc_decay) == 10.0 and int(Y.refrac) == 5
    assert float(Y.eps_0) == 1.0 and float(Y.rho_0) == 1.0 and float(Y.d_thresh) == 5.0 and Y.lbound is None
    Y.compute_decays(1.0)
    Y.set_batch_size(2)
    assert tuple(Y.v.shape) == (2, 3) and float(Y.v[0, 0]) == -70.0 and float(Y.decay) == float(torch.exp(-torch.tensor(1.0) / torch.tensor(10.0)))


def _rmax_net(B=1, conn="dense", target="srm0", additive=True):
    from bindsnet_amd.learning import Rmax
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, LIFNodes, SRM0Nodes
    from bindsnet_amd.network.topology import Connection
    net = Network(batch_size=B)
    X = Input(n=8, traces=True, traces_additive=additive)
    Y = SRM0Nodes(n=4, traces=True) if target == "srm0" else LIFNodes(n=4, traces=True)
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(Connection(X, Y, w=torch.rand(8, 4), update_rule=Rmax, nu=1e-3), "X", "Y")
    return net


def test_rmax_constructor_keeps_the_reference_assertions():
    with pytest.raises(AssertionError, match="additive spike traces"):
        _rmax_net(additive=False)
    with pytest.raises(AssertionError, match="SRM0Nodes"):
        _rmax_net(target="lif")
    net = _rmax_net()
    rule = net.connections[("X", "Y")].update_rule
    assert float(rule.tc_c) == 5.0 and float(rule.tc_e_trace) == 25.0 and not hasattr(rule, "eligibility_trace")


def test_rmax_at_batch_two_raises_before_the_run_changes_any_state():
    net = _rmax_net(B=2)
    v0, w0, st = net.layers["Y"].v.clone(), net.connections[("X", "Y")].w.clone(), torch.get_rng_state()
    with pytest.raises(NotImplementedError, match=r"view\(-1\)"):
        net.run({"X": torch.ones(3, 2, 8, dtype=torch.uint8)}, time=3, reward=1.0)
    assert torch.equal(net.layers["Y"].v, v0) and torch.equal(net.connections[("X", "Y")].w, w0)
    assert torch.equal(torch.get_rng_state(), st)


def test_rmax_takes_a_scalar_reward_only():
    net = _rmax_net()
    with pytest.raises(NotImplementedError, match="scalar reward"):
        net.run({"X": torch.ones(2, 1, 8, dtype=torch.uint8)}, time=2, reward=torch.ones(2))
    net = _rmax_net()
    torch.manual_seed(3)
    net.run({"X": torch.ones(2, 1, 8, dtype=torch.uint8)}, time=2, reward=torch.tensor([0.5]))
    assert tuple(net.connections[("X", "Y")].update_rule.eligibility_trace.shape) == (8, 4)


def test_rmax_on_other_connection_families_raises():
    from bindsnet_amd.learning import Rmax
    from bindsnet_amd.network.nodes import Input, SRM0Nodes
    from bindsnet_amd.network.topology import Conv2dConnection, MulticompartmentConnection, SparseConnection
    from bindsnet_amd.network.topology_features import Weight
    X = Input(shape=(1, 6, 6), traces=True, traces_additive=True)
    with pytest.raises(NotImplementedError):
        Conv2dConnection(X, SRM0Nodes(shape=(2, 4, 4), traces=True), kernel_size=3, update_rule=Rmax, nu=1e-3)
    X1 = Input(n=8, traces=True, traces_additive=True)
    with pytest.raises(NotImplementedError):
        SparseConnection(X1, SRM0Nodes(n=4), w=torch.rand(8, 4), update_rule=Rmax, nu=1e-3)
    mcc = MulticompartmentConnection(X1, SRM0Nodes(n=4), device="cpu", pipeline=[Weight("weight", torch.rand(8, 4))])
    with pytest.raises(NotImplementedError, match="not supported for this Connection type"):
        Rmax(connection=mcc, nu=1e-3)


def test_tensor_eps_0_is_refused_by_name_on_the_device_path():
    """The descriptor is what the device run is built from; it can be asked for without a GPU."""
    from bindsnet_amd import _lib
    from bindsnet_amd.network.nodes import SRM0Nodes
    for name in ("eps_0", "rho_0", "d_thresh", "rest", "reset"):
        Y = SRM0Nodes(n=4, **{name: torch.full((4,), 1.5)})
        Y.compute_decays(1.0)
        Y.set_batch_size(1)
        with pytest.raises(NotImplementedError, match=name):
            Y._describe(_lib.LayerDesc(), [], [])
    Y = SRM0Nodes(n=4, thresh=torch.full((4,), -51.0), tc_decay=torch.full((4,), 9.0), traces=True)
    Y.compute_decays(1.0)
    Y.set_batch_size(1)
    d, keep = _lib.LayerDesc(), []
    assert Y._describe(d, keep, []) > 0 and d.kind == _lib.LAYER_SRM0 and d.pv.v[0] and d.pv.v[1] and d.srm_sprob


def test_parallel_modes_name_the_layer_and_the_rule():
    from bindsnet_amd import parallel
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input
    from bindsnet_amd.network.topology import Connection
    plain = Network()
    plain.add_layer(Input(n=8), "X")
    plain.add_layer(SRM0Nodes(n=4), "Y")
    plain.add_connection(Connection(plain.layers["X"], plain.layers["Y"], w=torch.rand(8, 4)), "X", "Y")
    for net, what in ((plain, "SRM0Nodes"), (_rmax_net(), "Rmax")):
        with pytest.raises(NotImplementedError, match=what):
            parallel.column_shard(net, 0, 2)
        with pytest.raises(NotImplementedError, match=what):
            parallel.exact_run(net, {"X": torch.zeros(2, 1, 8, dtype=torch.uint8)}, time=2)
        with pytest.raises(NotImplementedError, match=what):
            parallel.sharded_run(net, {"X": torch.zeros(2, 1, 8, dtype=torch.uint8)}, time=2)
