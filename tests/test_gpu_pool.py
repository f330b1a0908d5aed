"""MaxPool1d / 2d / 3dConnection and MeanFieldConnection on the MI355X, bit for bit.

* Every fixture case of tests/golden/make_golden_pool.py (tests/pool_cases.py) through Network.run on the device, on the generic plan
  (the only plan such a graph takes), against the reference's recorded rasters, states, firing rates and learned weights; the same
  with every input run as two halves.
* ops.prop_pool (csrc/snn_pool.hip) against torch's own expressions on the host, over several steps from random rates, with and
  without `accumulate`; firing_rates and out sit in front of guard elements that must stay untouched.  The limits the shapes straddle:
    - 256 threads per workgroup: a pooled plane of 400 positions ([1,40,40] k2) and one of 9;
    - the window loops: a 7x7 window with stride 3 and padding 3, a dilated 3x3, 1-D and 3-D geometries;
    - SNN_POOL_STAGE = 8192 elements per staged plane: a plane of exactly 8192 ([64,128], the last one-launch form) and of 8256
      ([64,129], the first two-launch form); both forms must agree with the host and so with each other;
    - several planes per workgroup, G = min(8192 // plane, ceil(planes / 1024)): 3000 planes of 16 elements (G = 3, 1000 full
      groups) and 3001 of them (G = 3, 1001 groups, the last holding ONE plane: `np < G` in k_pool_staged); 7 planes of 3000
      elements run at G = 1 (fewer than 1024 planes always do);
    - the grid cap of 1024 workgroups: 5200 planes of 1600 elements (G = 5: 1040 plane groups, staged form) and 150 planes of 8256
      (1200 workgroups' worth of pooled positions, global form).
* ops.prop_meanfield against torch's mean: one element, no spike, every element spiking, element counts that are no multiple of the
  64-lane wave or of the 4-byte word, a spike pointer that is not 4-byte aligned, B * n_tgt beyond one workgroup (256) and beyond
  the 64-workgroup grid (16384), 0-dim / [n] / [B, n] weights, the three accumulate modes (a zero keeps its sign only in STORE).
* compute() by hand, reset_state_variables(), network.to("cuda") and what is refused."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_cases as PC
from test_pool_host import _bits, _ns, _same, _state, check_snapshots

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", PC.CASES)
def test_device_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    net = PC.build(_ns(), name).to(DEV)
    pool = PC.pool_of(net)
    assert pool is None or pool.firing_rates.is_cuda
    snaps = PC.run_case(net, name, Monitor, device=DEV)
    assert net.last_plan == "generic"
    check_snapshots(name, snaps)


@pytest.mark.parametrize("name", ["b", "e", "h", "m2"])
def test_two_halves_equal_one_whole_run_on_the_device(name):
    from bindsnet_amd.network.monitors import Monitor
    net = PC.build(_ns(), name).to(DEV)
    check_snapshots(name, PC.run_case(net, name, Monitor, device=DEV, split=True))
    assert net.last_plan == "generic"


SWEEP = [
    # (B, C, spatial, kernel, stride, padding, dilation)
    (2, 1, (40, 40), 2, 2, 0, 1),                   # a pooled plane larger than one workgroup
    (2, 3, (6, 6), 2, 2, 0, 1),
    (2, 2, (20, 20), 7, 3, 3, 1),                   # 7x7 window
    (2, 2, (13, 11), 3, (2, 1), (1, 0), (2, 1)),
    (3, 5, (37,), 3, 2, 1, 1),                      # 1-D
    (2, 2, (5, 4, 6), (3, 2, 2), (1, 2, 2), 1, 1),  # 3-D
    (1, 3, (64, 128), 2, 2, 0, 1),                  # exactly SNN_POOL_STAGE: staged
    (1, 3, (64, 129), 2, 2, 0, 1),                  # just past it: two launches
    (30, 100, (4, 4), 2, 1, 1, 1),                  # 3000 small planes: three per workgroup, 1000 full groups
    (1, 3001, (4, 4), 2, 1, 1, 1),                  # 3001: G = 3, the 1001st group holds one plane
    (2, 1025, (3, 5), 2, 1, 0, 1),                  # 2050 planes: G = 3, 684 groups, the last holds one plane
    (1, 7, (50, 60), 3, 2, 1, 1),                   # 7 large planes: one per workgroup (G = 1)
    (26, 200, (40, 40), 2, 2, 0, 1),                # 1040 plane groups: beyond the grid cap, staged form
    (3, 50, (64, 129), 2, 2, 0, 1),                 # beyond the grid cap, global form
]


GUARD = 7.0


def _guarded(host):
    """A device copy of `host` with 4096 guard elements behind it, and the guard: a write past the tensor's end shows there."""
    buf = torch.full((host.numel() + 4096,), GUARD, device=DEV)
    t = buf[:host.numel()].view(host.shape)
    t.copy_(host)
    return t, buf[host.numel():]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "x".join(str(v) for v in (c[0], c[1], *c[2])) + f"_k{c[3]}")
def test_prop_pool_equals_torch_on_the_host(case):
    from bindsnet_amd import ops
    B, C, spatial, k, s, p, d = case
    nd = len(spatial)
    pool = getattr(F, f"max_pool{nd}d")
    g = torch.Generator().manual_seed(B * 1000 + C + spatial[0])
    fr_h = 3.0 * torch.rand(B, C, *spatial, generator=g)
    fr_h[0, 0].zero_()                                        # a plane of ties
    fr_d, fr_guard = _guarded(fr_h)
    steps = 2 if B * C * int(np.prod(spatial)) > 1_000_000 else 4
    for step in range(steps):
        spikes = (torch.rand(B, C, *spatial, generator=g) < 0.4).to(torch.uint8)
        fr_h -= 0.3 * fr_h
        fr_h += spikes.float()
        _, idx = pool(fr_h, kernel_size=k, stride=s, padding=p, dilation=d, return_indices=True)
        want = spikes.flatten(2).gather(2, idx.flatten(2)).view_as(idx).float()
        accumulate = step % 2 == 1
        prev = torch.rand(want.shape, generator=g)
        out, out_guard = _guarded(prev)
        ops.prop_pool(fr_d, spikes.to(DEV), out, k, s, p, d, decay=0.3, accumulate=accumulate)
        torch.cuda.synchronize()
        assert bool((fr_guard == GUARD).all()) and bool((out_guard == GUARD).all()), f"step {step}: a write behind firing_rates or out"
        assert np.array_equal(_bits(fr_d.cpu().numpy()), _bits(fr_h.numpy())), f"step {step}: firing rates differ"
        want = prev + want if accumulate else want
        bad = np.flatnonzero(_bits(out.cpu().numpy()).reshape(-1) != _bits(want.numpy()).reshape(-1))
        assert bad.size == 0, f"step {step}: {bad.size} of {want.numel()} pooled values differ (first {bad[:5]})"
        assert 0 < float(want.sum())


MEAN_SWEEP = [
    # (B, n_src, n_tgt, density)
    (1, 1, 1, 1.0), (1, 1, 3, 0.0), (2, 67, 5, 0.3), (3, 257, 70, 0.5), (1, 1003, 300, 0.0), (2, 1003, 300, 1.0),
    (4, 5001, 5000, 0.2), (16, 6400, 6400, 0.05), (1, 1 << 24, 2, 0.1),
]


@pytest.mark.parametrize("case", MEAN_SWEEP, ids=lambda c: "x".join(str(v) for v in c[:3]) + f"_d{c[3]}")
def test_prop_meanfield_equals_torch_mean(case):
    from bindsnet_amd import ops
    B, n_src, n_tgt, density = case
    g = torch.Generator().manual_seed(n_src + n_tgt)
    full = torch.zeros(B * n_src + 1, dtype=torch.uint8)
    if density >= 1.0:
        full.fill_(1)
    elif density > 0.0:
        full.copy_(torch.rand(full.shape, generator=g) < density)
    full_d = full.to(DEV)
    for offset in (0, 1):                                     # (offset 1: the spike pointer is not 4-byte aligned)
        s = full[offset:offset + B * n_src].view(B, n_src)
        s_d = full_d[offset:offset + B * n_src].view(B, n_src)
        mean = s.float().mean()
        assert float(mean) == float(np.float32(int(s.sum())) / np.float32(s.numel()))
        for w in (torch.tensor(-0.5), torch.rand(n_tgt, generator=g) - 0.5, torch.rand(B, n_tgt, generator=g) - 0.5):
            prev = torch.rand(B, n_tgt, generator=g)
            for mode, want in (("store", (mean * w).expand(B, n_tgt)), ("first", torch.zeros(B, n_tgt) + mean * w), ("add", prev + mean * w)):
                out = prev.to(DEV)
                ops.prop_meanfield(w.to(DEV), s_d, out, accumulate=mode == "add", store=mode == "store")
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want.contiguous().numpy()).reshape(-1))
                assert bad.size == 0, f"offset {offset}, w {tuple(w.shape)}, {mode}: {bad.size} of {got.size} differ (first {bad[:5]})"


def test_compute_by_hand_reset_and_move():
    ns = _ns()
    host_net, dev_net = PC.build(ns, "b"), PC.build(ns, "b").to(DEV)
    ch, cd = PC.pool_of(host_net), PC.pool_of(dev_net)
    assert cd.firing_rates.is_cuda and tuple(cd.firing_rates.shape) == tuple(ch.firing_rates.shape)
    x = torch.from_numpy(PC.inputs("b", 0))
    for t in range(3):
        want, got = ch.compute(x[t]), cd.compute(x[t].to(DEV))
        assert got.is_cuda and got.shape == want.shape and np.array_equal(_bits(got.cpu().numpy()), _bits(want.numpy()))
        assert np.array_equal(_bits(cd.firing_rates.cpu().numpy()), _bits(ch.firing_rates.numpy()))
    ptr = cd.firing_rates.data_ptr()
    dev_net.reset_state_variables()
    assert cd.firing_rates.data_ptr() == ptr and not cd.firing_rates.any()
    s = torch.from_numpy(PC.inputs("m1", 0))[0]
    for w in (torch.tensor(-0.5), torch.arange(20.0) - 3.0):
        for spikes in (s, torch.zeros_like(s)):                # (no spike and w < 0: -0.0, as in the reference)
            mh = ns.MeanFieldConnection(ns.Input(n=50), ns.LIFNodes(n=20), w=w.clone())
            md = ns.MeanFieldConnection(ns.Input(n=50), ns.LIFNodes(n=20), w=w.clone()).to(DEV)
            want, got = mh.compute(spikes), md.compute(spikes.to(DEV))
            assert got.is_cuda and got.shape == want.shape and np.array_equal(_bits(got.cpu().numpy()), _bits(want.numpy()))


def test_built_before_its_layers_and_training_mode_run_on_the_device():
    ns = _ns()
    for make in (lambda: PC._pool_net(ns, (2, 4, 4), 2, before=True), lambda: PC._train(PC._pool_net(ns, (2, 4, 4), 2))):
        host_net, dev_net = make(), make().to(DEV)
        x = torch.from_numpy((np.random.default_rng(5).random((6, 2, 2, 4, 4)) < 0.5).astype(np.uint8))
        host_net.run({"X": x.clone()}, time=6)
        dev_net.run({"X": x.to(DEV)}, time=6)
        assert dev_net.last_plan == "generic"
        for a, b in zip(_state(host_net), _state(dev_net)):
            if a.dtype == torch.float32:
                assert np.array_equal(_bits(a.numpy()), _bits(b.cpu().numpy()))


def test_refusals_on_the_device_leave_the_state_alone():
    ns = _ns()
    x2 = lambda shape, B=2: {"X": torch.ones(3, B, *shape, dtype=torch.uint8, device=DEV)}       # noqa: E731
    mask = {("X", "Y"): torch.zeros(1, dtype=torch.bool)}
    for make, x, kwargs, exc, match in (
            (lambda: PC._pool_net(ns, (2, 4, 4), 2, decay=None), x2((2, 4, 4)), {}, TypeError, "decay"),
            (lambda: PC._pool_net(ns, (1, 4, 4), 2), x2((1, 4, 4)), {}, RuntimeError, "squeeze"),
            (lambda: PC._pool_net(ns, (2, 4, 4), 2, target=(8,)), x2((2, 4, 4)), {}, RuntimeError, "target's shape"),
            (lambda: PC._pool_net(ns, (2, 4, 4), 2), x2((2, 4, 4)), {"masks": mask}, NotImplementedError, "mask"),
            (lambda: PC._mean_net(ns, w=torch.tensor(0.5), norm=1.0), x2((6,)), {}, NotImplementedError, "TypeError"),
            (lambda: PC._mean_net(ns, w=torch.tensor(0.5)), x2((6,)), {"masks": mask}, NotImplementedError, "mask")):
        net = make().to(DEV)
        before = _state(net)
        with pytest.raises(exc, match=match):
            net.run(dict(x), time=3, **kwargs)
        assert _same(before, _state(net)), match


def test_a_refusal_at_another_batch_size_leaves_the_network_as_it_was_and_the_mended_run_equals_the_host():
    """Input (2, 4, 4) -> MaxPool2dConnection(2, stride 2) without `decay` -> LIFNodes (2, 2, 2), built at batch size 1 and run at 3:
    the TypeError comes before the batch size changes.  With decay=1.0 the same call runs, and its spikes are the host path's.
    (Two channels: with one, [3, 1, 4, 4] is what the reference's squeeze() cannot broadcast, and the run stays refused.  The
    connection is built before its layers join the network, so its rates take the run's batch size at first use.)"""
    from bindsnet_amd.network.monitors import Monitor
    ns = _ns()
    x = torch.from_numpy((np.random.default_rng(11).random((12, 3, 2, 4, 4)) < 0.5).astype(np.uint8))
    spikes = {}
    for dev in (DEV, "cpu"):
        net = PC._pool_net(ns, (2, 4, 4), 1, decay=None, before=True)
        net.layers["Y"].thresh.fill_(-64.5)                     # (a pooled spike or two per step must be enough to fire)
        net.add_monitor(Monitor(net.layers["Y"], ["s"], time=12), "Y")
        net = net.to(dev)
        Y = net.layers["Y"]
        v0 = Y.v.clone()
        with pytest.raises(TypeError, match="needs `decay=`"):
            net.run({"X": x.to(dev)}, time=12)
        assert net.batch_size == 1 and Y.v.shape[0] == 1 and torch.equal(Y.v, v0) and net.monitors["Y"].clean
        net.connections[("X", "Y")].decay = 1.0
        net.run({"X": x.to(dev)}, time=12)
        assert net.batch_size == 3 and Y.v.shape[0] == 3 and net.last_plan == ("generic" if dev == DEV else "host-torch")
        spikes[dev] = net.monitors["Y"].get("s").cpu()
    assert spikes[DEV].shape == (12, 3, 2, 2, 2) and int(spikes["cpu"].sum()) > 0
    assert torch.equal(spikes[DEV].to(torch.uint8), spikes["cpu"].to(torch.uint8))
