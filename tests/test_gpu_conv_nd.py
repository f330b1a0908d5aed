"""Conv1dConnection / Conv3dConnection with PostPre on the MI355X, bit for bit.

* Every fixture case of tests/golden/make_golden_conv_nd.py (tests/conv_nd_cases.py) on the device over its consecutive
  inputs, on the generic plan (the only plan such a graph takes); two half runs == one whole run; a weight monitor on a
  Conv1dConnection.
* Device-versus-host sweeps of the two kernels (csrc/snn_convnd.hip) and of compute() against their order contracts
  (_seq_conv; the reference's PostPre expressions of network/host_path.py with _seq_bmm).  The limits they straddle:
    - k_prop_convnd: 256 threads, tiles of nco channels x PB <= 256 positions (27, 64 and 300 positions: not multiples of the
      workgroup); filters staged in 48 KiB of LDS where Cin*K <= 12288 (K = 16384 reads them from L2); a sample's bitstream
      staged in 16 KiB where n_src <= 131072 (140 000 packs it from global memory); kernel_prod 1, 56, 4096; Cin 1/2/16.
    - k_convnd_postpre: 256 threads, at most 4096 workgroups, grid-stride over Cout*Cin*K (1.2 M elements > 4096 * 256);
      target masks staged in 32 KiB of LDS where B*Cout*ceil(L/32) <= 8192 words, else packed to scratch; batch sums over
      B = 1 / 3 / 33 in ATen's column classes; padding entries of the gather table."""
import numpy as np
import pytest
import torch

import conv_nd_cases as CC
from test_conv_nd_host import _bits, _ns, check_snapshots

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run_device(name, first=0, count=None):
    from bindsnet_amd.network.monitors import Monitor
    net = CC.build(_ns(), name).to(DEV)
    snaps = CC.run_case(net, name, Monitor, device=DEV, first=first, count=count)
    return net, snaps


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_device_reproduces_reference_fixture(name):
    net, snaps = _run_device(name)
    assert net.last_plan == "generic"
    check_snapshots(name, snaps)


def test_consecutive_inputs_from_the_middle():
    """Inputs 1.. of case (a) from a fresh network equal nothing the fixture pins -- but a network that ran input 0 and then
    the rest in a second call is the same as one call over all inputs."""
    net, first = _run_device("a", 0, 1)
    from bindsnet_amd.network.monitors import Monitor
    rest = CC.run_case(net, "a", Monitor, device=DEV, first=1)
    check_snapshots("a", first + rest)


def test_two_half_runs_equal_one_whole_run():
    from bindsnet_amd.network.monitors import Monitor
    name = "b"
    T = CC.CASES[name]["T"]
    x = torch.from_numpy(CC.inputs(name, 0)).to(DEV)
    whole = CC.build(_ns(), name).to(DEV)
    halves = CC.build(_ns(), name).to(DEV)
    for n in (whole, halves):
        n.connections[("X", "Y")].norm = None            # normalisation runs after every call: not part of the split
    mw, mh = Monitor(whole.layers["Y"], ["s"], time=T), Monitor(halves.layers["Y"], ["s"], time=T // 2)
    whole.add_monitor(mw, "s")
    halves.add_monitor(mh, "s")
    rng = torch.get_rng_state()                        # both see the same one-spike draws of the global generator
    whole.run({"X": x}, time=T)
    torch.set_rng_state(rng)
    halves.run({"X": x[:T // 2]}, time=T // 2)
    first = mh.get("s").clone()
    mh.reset_state_variables()
    halves.run({"X": x[T // 2:]}, time=T // 2)
    assert whole.last_plan == halves.last_plan == "generic"
    assert torch.equal(mw.get("s"), torch.cat([first, mh.get("s")]))
    a, b = CC.snapshot(whole, np.zeros(1)), CC.snapshot(halves, np.zeros(1))
    for k in ("v", "refrac", "theta", "xX", "xY", "w"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_weight_monitor_on_conv1d_connection():
    """Monitor(conn, ['w']) records w at the end of every step: equal to the host path's monitor, step by step."""
    from bindsnet_amd.network.monitors import Monitor
    name = "b"
    T = CC.CASES[name]["T"]
    x = torch.from_numpy(CC.inputs(name, 0))
    out = []
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for dev in ("cpu", DEV):
            net = CC.build(_ns(), name).to(dev)
            mon = Monitor(net.connections[("X", "Y")], ["w"], time=T)
            net.add_monitor(mon, "w")
            net.run({"X": x.to(dev)}, time=T)
            out.append(mon.get("w").cpu().numpy())
    finally:
        torch.set_num_threads(n)
    assert out[0].shape == (T, 4, 2, 6)
    assert np.array_equal(_bits(out[0]), _bits(out[1]))
    assert not np.array_equal(out[1][0], out[1][-1])


# ---- kernel sweeps: device vs the reference's torch expressions on the host -----------------------------------------------
def _conn(kind, Cin, spatial, k, s, p, Cout, B, nu=(0.0, 0.0), wmin=None, wmax=None, weight_decay=0.0, seed=0):
    from bindsnet_amd.learning.learning import PostPre
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input
    from bindsnet_amd.network.topology import Conv1dConnection, Conv3dConnection
    torch.manual_seed(seed)
    out = [(n - k + 2 * p) // s + 1 for n in spatial]
    X, Y = Input(shape=[Cin, *spatial], traces=True), DiehlAndCookNodes(shape=[Cout, *out], traces=True)
    kw = {} if wmin is None else {"wmin": wmin}
    if wmax is not None:
        kw["wmax"] = wmax
    cls = Conv1dConnection if kind == "c1" else Conv3dConnection
    c = cls(X, Y, kernel_size=k, stride=s, padding=p, nu=nu, update_rule=PostPre, weight_decay=weight_decay,
            reduction=torch.squeeze if B == 1 else torch.sum, **kw)
    X.set_batch_size(B)
    Y.set_batch_size(B)
    c.w.data = (c.w.data - 0.3) * 2.0                  # signed weights
    c.b.data = torch.rand(Cout) - 0.5
    return c


# The witnesses of the sweeps are the ORDER CONTRACTS, written out in float32 numpy (one rounding per * and +): oneDNN's conv
# and bmm kernels on the CPU of the machine running this file need not be the build container's, where
# tests/test_conv_nd_host.py pins these same orders to F.conv1d / F.conv3d / torch.bmm and the fixtures were generated.
def _seq_conv(spk, W, bias, s, p):
    """F.conv1d / F.conv3d on 0/1 spikes: per output one sequential chain over the taps ascending, channel innermost, + bias."""
    nd = W.dim() - 2
    x = np.pad(spk.numpy().astype(np.float32), [(0, 0), (0, 0)] + [(p, p)] * nd)
    w = W.numpy().astype(np.float32)
    out_sz = [(x.shape[2 + i] - w.shape[2 + i]) // s + 1 for i in range(nd)]
    acc = np.zeros((spk.shape[0], w.shape[0], *out_sz), np.float32)
    for tap in np.ndindex(*w.shape[2:]):
        for ci in range(w.shape[1]):
            sl = tuple(slice(t, t + s * (o - 1) + 1, s) for t, o in zip(tap, out_sz))
            xv = x[(slice(None), ci) + sl][:, None]
            wv = w[(slice(None), ci) + tap].reshape((1, -1) + (1,) * nd)
            acc = acc + wv * xv
    return torch.from_numpy(acc + bias.numpy().astype(np.float32).reshape((1, -1) + (1,) * nd))


def _seq_bmm(a, b):
    """torch.bmm as the reference's PostPre meets it: ascending over the inner dimension."""
    a, b = a.numpy().astype(np.float32), b.numpy().astype(np.float32)
    acc = np.zeros((a.shape[0], a.shape[1], b.shape[2]), np.float32)
    for l in range(a.shape[2]):
        acc = acc + a[:, :, l, None] * b[:, None, l, :]
    return torch.from_numpy(acc)


PROP = [  # kind, Cin, spatial, k, s, p, Cout, B, density
    ("c1", 1, (784,), 56, 28, 0, 25, 1, 0.05), ("c1", 1, (784,), 56, 28, 0, 25, 33, 0.3), ("c1", 2, (60,), 6, 2, 1, 4, 3, 0.2),
    ("c1", 16, (40,), 7, 3, 1, 3, 2, 0.3), ("c1", 1, (300,), 1, 1, 0, 5, 3, 0.5), ("c1", 1, (16384,), 16384, 1, 0, 3, 2, 0.1),
    ("c1", 1, (140000,), 4, 4, 0, 2, 1, 0.01), ("c1", 2, (599,), 2, 2, 0, 3, 1, 1.0), ("c1", 1, (50,), 5, 1, 2, 300, 2, 0.0),
    ("c3", 1, (28, 28, 28), 16, 4, 0, 25, 1, 0.03), ("c3", 1, (28, 28, 28), 16, 4, 0, 3, 3, 0.3), ("c3", 1, (6, 6, 6), 3, 2, 1, 2, 33, 0.5),
    ("c3", 1, (10, 9, 8), 1, 1, 0, 2, 1, 0.5), ("c3", 1, (12, 12, 12), 5, 3, 2, 7, 2, 1.0),
]


@pytest.mark.parametrize("case", PROP)
def test_prop_convnd_sweep(case):
    from bindsnet_amd import ops
    kind, Cin, spatial, k, s, p, Cout, B, d = case
    c = _conn(kind, Cin, spatial, k, s, p, Cout, B, seed=Cout + B)
    g = torch.Generator().manual_seed(sum(spatial) + B)
    spk = (torch.rand(B, *c.source.shape, generator=g) < d).to(torch.uint8)
    want = _seq_conv(spk, c.w.data, c.b.data, s, p)
    out = torch.full((B, *c.target.shape), float("nan"), device=DEV)
    ops.prop_convnd(c.w.data.to(DEV), spk.to(DEV), out, bias=c.b.data.to(DEV), stride=s, pad=p)
    got = out.cpu()
    assert np.array_equal(_bits(got.numpy()), _bits(want.numpy())), \
        f"prop_convnd differs at {np.flatnonzero(_bits(got.numpy()) != _bits(want.numpy()))[:5]}"
    acc = out.clone()
    ops.prop_convnd(c.w.data.to(DEV), spk.to(DEV), acc, bias=c.b.data.to(DEV), stride=s, pad=p, accumulate=True)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits((want + want).numpy()))
    c.to(DEV)                                          # compute() on the device: the same kernel
    assert np.array_equal(_bits(c.compute(spk.to(DEV)).cpu().numpy()), _bits(want.numpy()))


VARIANTS = [dict(nu=(1e-2, 2e-2)), dict(nu=(0.0, 3e-2), wmin=-0.5, wmax=0.7), dict(nu=(5e-2, 0.0), wmin=-0.1),
            dict(nu=(1e-2, 1e-2), wmax=0.4, weight_decay=0.01)]
PP = [  # kind, Cin, spatial, k, s, p, Cout, B, target density
    ("c1", 1, (784,), 56, 28, 0, 25, 1, 0.05), ("c1", 1, (784,), 56, 28, 0, 25, 33, 0.1), ("c1", 2, (60,), 6, 2, 1, 4, 3, 0.2),
    ("c1", 16, (40,), 7, 3, 1, 3, 2, 0.3), ("c1", 4, (1000,), 1000, 1, 0, 300, 2, 0.5), ("c1", 1, (8000,), 2, 2, 0, 3, 3, 0.3),
    ("c1", 1, (5,), 5, 1, 0, 1, 33, 1.0), ("c1", 1, (1,), 1, 1, 0, 1, 33, 1.0), ("c1", 1, (70,), 3, 1, 2, 300, 33, 0.05),
    ("c3", 1, (28, 28, 28), 16, 4, 0, 25, 1, 0.02), ("c3", 1, (6, 6, 6), 3, 2, 1, 3, 33, 0.3), ("c3", 1, (9, 9, 9), 3, 2, 0, 5, 3, 0.5),
]


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("case", PP)
def test_convnd_postpre_sweep(case, variant, monkeypatch):
    from bindsnet_amd import ops
    from bindsnet_amd.network import host_path
    kind, Cin, spatial, k, s, p, Cout, B, d = case
    v = dict(VARIANTS[variant])
    if kind == "c3" and v["nu"][0] != 0.0:
        v["nu"] = (0.0, v["nu"][1] or 1e-2)            # the only conv3d PostPre the reference defines
    c = _conn(kind, Cin, spatial, k, s, p, Cout, B, seed=Cout + variant, **v)
    rule = c.update_rule
    g = torch.Generator().manual_seed(B * 13 + variant)
    c.source.s = (torch.rand(B, *c.source.shape, generator=g) < 0.3).view(B, *c.source.shape)
    c.target.s = (torch.rand(B, *c.target.shape, generator=g) < d).view(B, *c.target.shape)
    c.source.x = torch.rand(B, *c.source.shape, generator=g) * (torch.rand(B, *c.source.shape, generator=g) < 0.6)
    c.target.x = torch.rand(B, *c.target.shape, generator=g) * (torch.rand(B, *c.target.shape, generator=g) < 0.6)
    W = c.w.data.clone().to(DEV)
    lo, hi = rule._bounds()
    ops.convnd_postpre(W, c.pp_src.to(DEV), c.source.s.reshape(B, -1).to(DEV).to(torch.uint8), c.source.x.reshape(B, -1).to(DEV),
                       c.target.s.reshape(B, -1).to(DEV).to(torch.uint8), c.target.x.reshape(B, -1).to(DEV), float(rule.nu[0]),
                       float(rule.nu[1]), decay=float(rule.weight_decay), wmin=lo, wmax=hi)
    monkeypatch.setattr(torch, "bmm", _seq_bmm)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        host_path._update_convnd(c, rule)
    finally:
        torch.set_num_threads(n)
    got, want = _bits(W.cpu().numpy()).reshape(-1), _bits(c.w.data.numpy()).reshape(-1)
    assert np.array_equal(got, want), f"convnd_postpre differs at {np.flatnonzero(got != want)[:5]}"


def test_masks_and_conv3d_nu0_raise_on_the_device():
    from bindsnet_amd.network.monitors import Monitor  # noqa: F401
    net = CC.build(_ns(), "a").to(DEV)
    with pytest.raises(NotImplementedError, match="masks"):
        net.run({"X": torch.zeros(4, 1, 1, 784, dtype=torch.uint8, device=DEV)}, time=4,
                masks={("X", "Y"): torch.zeros(25, 1, 56, dtype=torch.bool)})
    net3 = CC.build(_ns(), "g").to(DEV)
    net3.train(True)
    conn = net3.connections[("X", "Y")]
    w0 = conn.w.detach().clone()
    with pytest.raises(RuntimeError, match="float != bool"):
        net3.run({"X": torch.zeros(4, 1, 1, 28, 28, 28, dtype=torch.uint8, device=DEV)}, time=4)
    assert torch.equal(conn.w, w0)
