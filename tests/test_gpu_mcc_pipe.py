"""MulticompartmentConnection feature pipelines on the MI355X (csrc/snn_mccpipe.hip), bit for bit.

  * every reference-generated fixture case of tests/mcc_pipe_cases.py on the device, generic plan: rasters, final state, feature
    values and the HOST generator's state after every run (the Bernoulli draws are taken from its stream on the device);
  * against the host path (network/host_path.py, pinned to the same fixtures by tests/test_mcc_pipe_host.py): a sweep of shapes
    that cross the kernels' boundaries, a hand call of compute(), case (a) inside Network.pipelined();
  * ops.mcc_bernoulli against torch.bernoulli on the CPU from the same seed; what raises."""
import numpy as np
import pytest
import torch

import mcc_pipe_cases as PC
from test_mcc_pipe_host import _bits, _ns, build, check_snapshots, gold

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def few_host_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(4, n))
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_device_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    net = build(name).to(DEV)
    snaps = PC.run_case(net, name, Monitor, device=DEV)
    assert net.last_plan == "generic"
    assert sum(int(v.sum()) for s in snaps for k, v in s.items() if k.startswith("raster_")) == int(gold(name)["spikes"])
    check_snapshots(name, snaps)


def _ff(pipe, S, N, seed, wscale):
    """Input S -> pipeline -> LIF N with the cases' value generators."""
    ns = _ns()
    c = dict(pipe=pipe, wscale=wscale)
    rng = np.random.default_rng(seed)
    net = ns.Network(dt=1.0)
    X, Y = ns.Input(n=S, traces=True), ns.LIFNodes(n=N, traces=True)
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(ns.MulticompartmentConnection(X, Y, device="cpu", pipeline=PC.make_pipeline(ns, c, S, N, "in", rng)), "X", "Y")
    return net


def _run_both(make, x, T, seed):
    from bindsnet_amd.network.monitors import Monitor
    out = {}
    for dev in ("cpu", DEV):
        net = make()
        mon = Monitor(net.layers["Y"], ["s", "v"], time=T)
        net.add_monitor(mon, "Y")
        net.to(dev)
        torch.manual_seed(seed)
        torch.rand(seed % 7)                       # (the run starts somewhere inside a 624-word block)
        net.run({"X": torch.from_numpy(x.copy()).to(dev)}, time=T)
        out[dev] = dict(s=mon.get("s").cpu().numpy().astype(np.uint8), v=mon.get("v").cpu().numpy(), rng=torch.get_rng_state().numpy().copy(),
                        plan=net.last_plan, x=net.layers["Y"].x.cpu().numpy())
    return out


SWEEP = [("PW", 17, 31), ("PW", 39, 16), ("PW", 19, 33), ("PWB", 15, 32), ("PW", 16, 70), ("PW", 17, 64), ("PMW", 255, 33), ("PW", 256, 31),
         ("PWB", 257, 65), ("PPW", 1040, 3), ("WB", 300, 257), ("P", 40, 300)]


@pytest.mark.parametrize("pipe,S,N", SWEEP)
def test_device_equals_the_host_path_across_kernel_boundaries(pipe, S, N):
    """S*N below / at / above 624 and no multiple of it; N = 31 / 32 / 33 / 64 / 65 / 70 / 257 / 300 (bit-row padding, more than one
    block of columns, the cascade / row_sum split); S on both sides of 16 and 256 and past 1024 (the list chunks of the sparse walk)."""
    T, B = 8, 3
    x = (np.random.default_rng(S + N).random((T, B, S)) < min(0.5, 12.0 / S)).astype(np.uint8)
    out = _run_both(lambda: _ff(pipe, S, N, S * N, 30.0 / max(4.0, 0.25 * min(S, 48))), x, T, S + N)
    h, d = out["cpu"], out[DEV]
    assert (h["plan"], d["plan"]) == ("host-torch", "generic")
    print(f"{pipe} S={S} N={N}: host spikes {int(h['s'].sum())}, device spikes {int(d['s'].sum())}, v elements that differ "
          f"{int((_bits(h['v']) != _bits(d['v'])).sum())} of {h['v'].size}")
    assert h["s"].sum() > 0, "vacuous"
    assert np.array_equal(d["s"], h["s"]) and np.array_equal(_bits(d["v"]), _bits(h["v"])) and np.array_equal(_bits(d["x"]), _bits(h["x"]))
    assert np.array_equal(d["rng"], h["rng"]), "the device run leaves the host generator elsewhere"


def _pack(hits):
    S, N = hits.shape
    padded = np.zeros((S, (N + 31) // 32 * 32), np.uint8)
    padded[:, :N] = hits
    return np.ascontiguousarray(np.packbits(padded.reshape(S, -1, 32), axis=2, bitorder="little").view(np.uint32).reshape(S, -1))


@pytest.mark.parametrize("S,N", [(1, 1), (7, 89), (16, 39), (25, 25), (5, 251)])          # S*N = 1, 623, 624, 625, 1255
def test_mcc_bernoulli_equals_torch_bernoulli(S, N):
    from bindsnet_amd import ops
    for warm in (0, 620):
        torch.manual_seed(200 + S)
        p = torch.rand(S, N)
        if warm:
            torch.rand(warm)
        st = torch.get_rng_state()
        want = torch.bernoulli(p).numpy() != 0
        after = torch.get_rng_state()
        torch.set_rng_state(st)
        bits = ops.mcc_bernoulli(p.to(DEV), S, N).cpu().numpy().view(np.uint32).reshape(S, -1)
        assert np.array_equal(bits, _pack(want)), f"S*N = {S * N}, warm {warm}: mask differs from torch.bernoulli"
        assert torch.equal(torch.get_rng_state(), after), "the generator position afterwards is not torch's"
    torch.set_rng_state(st)
    one = ops.mcc_bernoulli(p.reshape(-1)[:1].contiguous().to(DEV), S, N).cpu().numpy().view(np.uint32).reshape(S, -1)
    torch.set_rng_state(st)
    assert np.array_equal(one, _pack(torch.bernoulli(p.reshape(-1)[:1].expand(S, N).contiguous()).numpy() != 0)), "scalar p"


def test_pipelined_section_gives_the_bits_of_synchronous_runs():
    from bindsnet_amd.network.monitors import Monitor
    c = PC.CASES["a"]
    rec = {}
    for mode in ("sync", "pipe"):
        net = build("a").to(DEV)
        mon = Monitor(net.layers["Y"], ["s"], time=c["T"])
        net.add_monitor(mon, "Y")
        xs = [torch.from_numpy(PC.inputs("a", r).copy()).to(DEV) for r in range(3)]
        got = []
        if mode == "pipe":
            with net.pipelined():
                for x in xs:
                    net.run({"X": x}, time=c["T"])
                    got.append(mon.get("s").clone())
                    net.reset_state_variables()
        else:
            for x in xs:
                net.run({"X": x}, time=c["T"])
                got.append(mon.get("s").clone())
                net.reset_state_variables()
        rec[mode] = ([g.cpu().numpy() for g in got], net.layers["Y"].v.cpu().numpy(), torch.get_rng_state().numpy().copy())
    for a, b in zip(rec["sync"][0], rec["pipe"][0]):
        assert a.sum() > 0 and np.array_equal(a, b)
    assert np.array_equal(_bits(rec["sync"][1]), _bits(rec["pipe"][1])) and np.array_equal(rec["sync"][2], rec["pipe"][2])
    g = gold("a")
    assert np.array_equal(np.packbits(rec["pipe"][0][1].astype(np.uint8).reshape(-1)), g["r1_raster_Y"])


@pytest.mark.parametrize("pipe", ["PW", "PMWB", "WP"])
def test_hand_call_of_compute_equals_the_host(pipe):
    S, N, B = 45, 37, 3
    s = (np.random.default_rng(3).random((B, S)) < 0.4).astype(np.uint8)
    res = {}
    for dev in ("cpu", DEV):
        net = _ff(pipe, S, N, 5, 2.0).to(dev)
        conn = net.connections[("X", "Y")]
        torch.manual_seed(9)
        res[dev] = [conn.compute(torch.from_numpy(s.copy()).to(dev)).cpu().numpy() for _ in range(3)] + [torch.get_rng_state().numpy().copy()]
    for a, b in zip(res["cpu"][:3], res[DEV][:3]):
        assert a.dtype == np.float32 and np.abs(a).sum() > 0 and np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(res["cpu"][3], res[DEV][3])


def test_what_raises_on_the_device():
    from bindsnet_amd import parallel
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Mask
    net = build("a").to(DEV)
    x = torch.zeros(2, 1, 36, dtype=torch.uint8, device=DEV)
    for mode in (lambda: parallel.column_shard(net, 0, 2), lambda: parallel.sharded_run(net, {"X": x}, 2), lambda: parallel.exact_run(net, {"X": x}, 2)):
        with pytest.raises(NotImplementedError, match=r"\['Probability', 'Weight'\]"):
            mode()
    conn = MulticompartmentConnection(Input(n=6), LIFNodes(n=5), device="cpu", pipeline=[Mask("m", torch.ones(6, 5, dtype=torch.bool))]).to(DEV)
    with pytest.raises(NotImplementedError, match="host path"):
        conn.compute(torch.ones(1, 6, dtype=torch.uint8, device=DEV))
