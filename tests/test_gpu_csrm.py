"""CSRMNodes on the MI355X (csrc/snn_csrm.hip): snn_prop_window_f32 and snn_csrm_step inside the generic plan.

The device cannot follow torch's einsum and matmul bit for bit (blocked BLAS orders), so the contract has two halves:
  1. the device equals the STATED ORDER (csrm_cases.stated_run: plain float32 torch, no package code) bit for bit -- v, s, theta,
     last_spikes, s_w, the traces and w;
  2. on every fixture the stated order's raster, theta, last_spikes, s_w, traces and learned weights are the reference's bit for
     bit and v stays within the fixture's measured `v_spread` (tests/test_csrm_host.py pins that half without a GPU; here the
     device is held to it directly as well).

Limits of the kernels, straddled by the sweeps below:
  * k_prop_window tiles the columns by 256 (one workgroup per tile, slot and sample): N = 1, 255, 257 and 600 (three tiles);
  * it compacts the spiking sources in chunks of 256: source sizes 50 (part of one chunk) and 784 (three chunks and a rest, no
    multiple of 16), a step with an empty window and a step in which every source spiked (a full 256-entry list);
  * the ring: windows of 1 (the pushed slot is the only one), 20 and 33 (more than 32) slots, more steps than slots so that the
    head wraps;
  * k_csrm_step loops the batch per neuron: B = 1 and 3;
  * SNN_CSRM_MAX_WINDOW = 1024 slots and B * window * n < 2^31 are refused in Python before any launch."""
import numpy as np
import pytest
import torch

import csrm_cases as CC
from test_csrm_host import _ns, build, check_snapshots, decays, gold, same

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEVICE_CASES = sorted(n for n in CC.CASES if n not in CC.HOST_ONLY)


@pytest.fixture(autouse=True)
def few_host_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def stated():
    """The stated order of every fixture case, computed once (per-step v included)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    out = {name: CC.stated_run(CC.CASES[name], int(gold(name)["seed"]), record_v=True, decays=decays(name)) for name in DEVICE_CASES}
    torch.set_num_threads(n)
    return out


def run_device(name, **kw):
    from bindsnet_amd.network.monitors import Monitor
    net = build(name).to(DEV)
    snaps = CC.run_case(net, CC.CASES[name], int(gold(name)["seed"]), Monitor, device=DEV, **kw)
    assert net.last_plan == "generic"
    return net, snaps


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_device_equals_stated_order_and_reference_fixture(name, stated):
    net, snaps = run_device(name)
    for r, s in enumerate(snaps):
        d = float(np.abs(s["v"].astype(np.float64) - gold(name)[f"r{r}_v"].astype(np.float64)).max())
        print(f"case {name} input {r}: |v - reference| = {d:.3g} (v_spread {float(gold(name)['v_spread']):.3g})")
    check_snapshots(name, snaps, against=stated[name], v_exact=True)       # half 1
    check_snapshots(name, snaps)                                           # half 2
    conn = net.connections[("X", "Y")]
    assert conn.s_w.dtype == torch.float32 and conn.s_w.is_cuda and net.layers["Y"].last_spikes.dtype == torch.float32


@pytest.mark.parametrize("name", ["learn100", "b3_postpre", "two_inputs", "recurrent", "win33_1", "win1_10", "pervec"])
def test_two_half_runs_equal_one_whole_run(name, stated):
    _, snaps = run_device(name, halves=True)
    check_snapshots(name, snaps, against=stated[name], v_exact=True)


@pytest.mark.parametrize("name", ["b3_postpre", "lbound", "two_conns"])
def test_voltage_monitor_step_by_step(name, stated):
    from bindsnet_amd.network.monitors import Monitor
    c, seed = CC.CASES[name], int(gold(name)["seed"])
    net = build(name).to(DEV)
    mon = Monitor(net.layers["Y"], ["v", "s"], time=c["T"])
    net.add_monitor(mon, name="Y_v")
    net.run({k: torch.from_numpy(a).to(DEV) for k, a in CC.inputs(c, seed, 0).items()}, time=c["T"], **CC.run_kwargs(c))
    assert net.last_plan == "generic"
    same(mon.get("v").cpu().numpy().reshape(c["T"], c["B"], c["N"]), stated[name][0]["vrec"], f"case {name}: per-step v")
    assert np.array_equal(mon.get("s").cpu().numpy().reshape(c["T"], c["B"], c["N"]).astype(np.uint8), stated[name][0]["raster"])


def test_moving_to_the_device_carries_the_windows(stated):
    """The first steps of an input on the host, network.to('cuda'), the rest on the device: s_w and last_spikes travel (the
    reference forgets s_w).  The split lies right behind a step with a spike, so last_spikes is not empty when it moves."""
    name = "two_inputs"
    c, seed, want = CC.CASES[name], int(gold(name)["seed"]), stated[name][0]
    assert float(gold(name)["v_spread"]) == 0.0            # (the host half runs torch's order: v is the stated order's only at spread 0)
    T = c["T"]
    h = max(t for t in range(5, T - 5) if want["raster"][t - 1].any())
    net = build(name)
    x = torch.from_numpy(CC.inputs(c, seed, 0)["X"])
    net.run({"X": x[:h]}, time=h)
    assert net.last_plan == "host-torch"
    conn, Y = net.connections[("X", "Y")], net.layers["Y"]
    s_w, last = conn.s_w.clone(), Y.last_spikes.clone()
    assert s_w.any() and last.any()
    net.to(DEV)
    assert conn.s_w.is_cuda and Y.last_spikes.is_cuda
    assert torch.equal(conn.s_w.cpu(), s_w) and torch.equal(Y.last_spikes.cpu(), last)
    net.run({"X": x[h:].to(DEV)}, time=T - h)
    assert net.last_plan == "generic"
    got = CC.snapshot(net, want["raster"])
    for k in ("v", "theta", "last", "s_w", "xX", "xY", "w"):
        same(got[k], want[k], f"{k} behind the move")


def test_clamp_unclamp_and_injected_voltage(stated):
    """run(clamp=, unclamp=, injects_v=) as for IFNodes: the injected voltage in front of the step, the clamps behind it -- behind
    the push into last_spikes, in front of PostPre."""
    from bindsnet_amd.network.monitors import Monitor
    name = "two_inputs"
    c, seed = CC.CASES[name], int(gold(name)["seed"])
    clamp, unclamp = torch.zeros(c["N"], dtype=torch.bool), torch.zeros(c["N"], dtype=torch.bool)
    clamp[1] = clamp[7] = unclamp[7] = unclamp[4] = True
    inject = torch.linspace(-0.5, 0.5, c["N"])
    want = CC.stated_run(c, seed, clamp=clamp, unclamp=unclamp, inject_v=inject)
    assert not np.array_equal(want[0]["raster"], stated[name][0]["raster"]) and not np.array_equal(want[1]["w"], stated[name][1]["w"])
    net = build(name).to(DEV)
    snaps = CC.run_case(net, c, seed, Monitor, device=DEV, clamp={"Y": clamp}, unclamp={"Y": unclamp}, injects_v={"Y": inject})
    assert net.last_plan == "generic"
    check_snapshots(name, snaps, against=want, v_exact=True)


def _device_state(net):
    Y, conn = net.layers["Y"], net.connections[("X", "Y")]
    return [t.clone() for t in (Y.v, Y.s, Y.x, Y.theta, Y.last_spikes, conn.w.data, conn.s_w)]


def test_device_only_refusals_leave_the_state_untouched():
    ns = _ns()
    net = CC._small(ns).to(DEV)
    x = CC._spikes(4, 1).to(DEV)
    net.run({"X": x}, time=4)
    before = _device_state(net)
    with pytest.raises(NotImplementedError, match=r"inputs\['Y'\]"):
        net.run({"X": x, "Y": torch.ones(4, 1, 5, device=DEV)}, time=4)
    for name in ("rest",):
        other = CC._small(ns, **{name: torch.full((5,), 3.0)}).to(DEV)
        v0 = other.layers["Y"].v.clone()
        with pytest.raises(NotImplementedError, match=name):
            other.run({"X": x}, time=4)
        assert torch.equal(other.layers["Y"].v, v0) and other.connections[("X", "Y")].s_w is None
    big = CC._small(ns, res_window_size=1025).to(DEV)
    with pytest.raises(NotImplementedError, match="limits"):
        big.run({"X": x}, time=4)
    with pytest.raises(RuntimeError):                      # a window made at batch size 1
        net.run({"X": CC._spikes(4, 2).to(DEV)}, time=4)
    for a, b in zip(before, _device_state(net)):
        assert torch.equal(a, b)
    net.run({"X": x}, time=4)                              # and the network still runs
    assert net.last_plan == "generic"


@pytest.mark.parametrize("Nin", [50, 784])
@pytest.mark.parametrize("B,Wn", [(1, 1), (3, 20), (1, 33)])
def test_window_propagation_sweep(B, Wn, Nin):
    from bindsnet_amd import ops
    rng = np.random.default_rng(B * 1000 + Wn + Nin)
    for N in (1, 255, 257, 600):
        W = torch.from_numpy(rng.standard_normal((Nin, N)).astype(np.float32))
        bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
        Wd, bd = W.to(DEV), bias.to(DEV)
        ring = torch.zeros(B, Wn, Nin, dtype=torch.uint8, device=DEV)
        window, head = torch.zeros(B, Wn, Nin), 0
        for t in range(Wn + 3):                    # step 0: nothing anywhere in the window; step 1: every source; then 20 %
            s = torch.from_numpy((rng.random((B, Nin)) < (0.0 if t == 0 else 1.0 if t == 1 else 0.2)).astype(np.uint8))
            window = torch.cat((window[:, 1:], s[:, None].float()), 1)
            before = torch.from_numpy(rng.standard_normal((B, Wn, N)).astype(np.float32))
            got = ops.prop_window(Wd, ring.clone(), head, s.to(DEV), torch.full((B, Wn, N), float("nan"), device=DEV), bias=bd)
            got_acc = ops.prop_window(Wd, ring, head, s.to(DEV), before.to(DEV), accumulate=True)
            head = (head + 1) % Wn
            same(got.cpu().numpy(), CC.window_currents(None, window, W, bias).numpy(), f"N {N} step {t}: window currents")
            same(got_acc.cpu().numpy(), CC.window_currents(before, window, W).numpy(), f"N {N} step {t}: accumulated window currents")
            same(torch.cat((ring[:, head:], ring[:, :head]), 1).float().cpu().numpy(), window.numpy(), f"N {N} step {t}: the ring")


@pytest.mark.parametrize("B,Wres,Wref", [(1, 1, 10), (3, 20, 10), (1, 33, 1), (3, 33, 33)])
def test_step_sweep(B, Wres, Wref):
    from bindsnet_amd import _lib, ops
    rng = np.random.default_rng(B * 100 + Wres)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))       # noqa: E731
    for N in (1, 255, 257, 600):
        for learning, vec, lbound in ((1, False, None), (0, True, -66.0)):
            resK, refK = f(Wres), -f(Wref).abs()
            thresh = torch.tensor(-64.0) if not vec else -64.0 + f(N)
            par = dict(decay=torch.tensor(0.99), theta_decay=torch.tensor(0.995), theta_plus=torch.tensor(0.5), thresh=thresh, lbound=lbound,
                       learning=bool(learning), trace_decay=torch.tensor(0.95))
            st = dict(v=-65.0 + f(B, N), theta=f(N).abs(), last=(f(B, Wref, N) > 0.5).float(), xtr=f(B, N).abs())
            p = _lib.DcParams()
            p.lif.decay, p.lif.thresh, p.lif.dt, p.lif.traces, p.lif.trace_decay, p.lif.trace_scale = 0.99, 0.0 if vec else -64.0, 1.0, 1, 0.95, 1.0
            p.lif.has_lbound, p.lif.lbound = int(lbound is not None), lbound or 0.0
            p.theta_decay, p.theta_plus, p.learning = 0.995, 0.5, learning
            dev = {k: t.to(DEV).contiguous() for k, t in st.items()}
            s = torch.zeros(B, N, dtype=torch.bool, device=DEV)
            spikes = 0
            for t in range(4):
                x = 2.0 * f(B, Wres, N)
                ops.csrm_step(dev["v"], s, dev["xtr"], dev["theta"], x.to(DEV), dev["last"], resK.to(DEV), refK.to(DEV), p,
                              pv={"thresh": thresh.to(DEV)} if vec else None)
                CC.csrm_step(st, x, resK, refK, par)
                spikes += int(st["s"].sum())
                assert torch.equal(s.cpu(), st["s"])
                for k in ("v", "theta", "last", "xtr"):
                    same(dev[k].cpu().numpy(), st[k].numpy(), f"N {N} step {t}: {k}")
            assert 0 < spikes < 4 * B * N or N == 1


@pytest.mark.parametrize("B,wres,src,N", [(3, 33, (784,), 257), (1, 20, (50,), 600)])
def test_network_sweep_against_the_stated_order(B, wres, src, N):
    from bindsnet_amd.network.monitors import Monitor
    c = dict(CC._BASE, src=src, N=N, B=B, T=wres + 4, wres=wres, rule="PostPre", nu=1e-2, density=0.05, wscale=4.0 / src[0] ** 0.5)
    net = CC.build(_ns(), c, 3).to(DEV)
    snaps = CC.run_case(net, c, 3, Monitor, device=DEV)
    assert net.last_plan == "generic"
    want = CC.stated_run(c, 3)
    for k in ("v", "theta", "last", "s_w", "xX", "xY", "w"):
        same(snaps[0][k], want[0][k], f"{k}")
    assert np.array_equal(snaps[0]["raster"], want[0]["raster"])
