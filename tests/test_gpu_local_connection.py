"""LocalConnection1D / 2D / 3D with PostPre and AdaptiveLIFNodes on the MI355X, bit for bit.

* Every fixture case of tests/golden/make_golden_local.py (tests/local_cases.py) on the device over its consecutive inputs,
  on the generic plan (the only plan a graph with a LOCAL connection takes); two half runs == one whole run; a weight
  monitor on a LocalConnection2D; AdaptiveLIFNodes behind a plain Connection on the automatic plan and the forced generic
  plan.
* Device-versus-host sweeps of the two kernels (csrc/snn_local.hip) against the reference's own torch expressions
  (network/host_path.py).  The per-workgroup limits they straddle:
    - k_prop_local: 256 threads per workgroup, one target neuron per thread in a stride loop over R = F*conv_prod, at most
      1024 workgroups per sample (R = 300 and 300 000 > 256 * 1024 go round the loops); one sample's spikes staged in
      32 KiB of LDS (n_src = 40 000 > 32 768 takes the global-memory form); inner-sum lanes of 8 (kernel_prod 1 and 7 < 8,
      144, 300, 1000 not multiples of 32).
    - k_local_postpre: 256 threads per workgroup, at most 4096 workgroups, grid-stride over the W.numel() elements
      (Cin 4 x kernel_prod 1000 x 300 filters = 1.2 M > 4096 * 256); batch sums over B = 33 > 32 terms in each of ATen's
      column classes (cascade below 32*floor(numel/32), row_sum above; the narrow special cases numel = 1 and 4..7).
* The rules that are not supported raise."""
import copy

import numpy as np
import pytest
import torch

import local_cases as LC
from test_local_connection_host import _bits, _ns, check_snapshots

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run_device(name, first=0, count=None, net=None):
    from bindsnet_amd.network.monitors import Monitor
    if net is None:
        net = LC.build(_ns(), name)
        net.to(DEV)
    snaps = LC.run_case(net, name, Monitor, device=DEV, first=first, count=count)
    return net, snaps


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_device_reproduces_reference_fixture(name):
    net, snaps = _run_device(name)
    if name != "f":
        assert net.last_plan == "generic"
    check_snapshots(name, snaps)


def test_two_half_runs_equal_one_whole_run():
    from bindsnet_amd.network.monitors import Monitor
    name = "b"
    T = LC.CASES[name]["T"]
    x = torch.from_numpy(LC.inputs(name, 0)).to(DEV)
    whole = LC.build(_ns(), name).to(DEV)
    halves = LC.build(_ns(), name).to(DEV)
    mw, mh = Monitor(whole.layers["Y"], ["s"], time=T), Monitor(halves.layers["Y"], ["s"], time=T // 2)
    whole.add_monitor(mw, "s")
    halves.add_monitor(mh, "s")
    whole.run({"X": x}, time=T)
    halves.run({"X": x[:T // 2]}, time=T // 2)
    first = mh.get("s").clone()
    mh.reset_state_variables()
    halves.run({"X": x[T // 2:]}, time=T // 2)
    assert whole.last_plan == halves.last_plan == "generic"
    assert torch.equal(mw.get("s"), torch.cat([first, mh.get("s")]))
    a, b = LC.snapshot(whole, np.zeros(1)), LC.snapshot(halves, np.zeros(1))
    for k in ("v", "refrac", "theta", "xX", "xY", "w"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_weight_monitor_on_local_connection_2d():
    """Monitor(conn, ['w']) records w at the end of every step: equal to the host path's monitor, step by step."""
    from bindsnet_amd.network.monitors import Monitor
    name = "b"
    T = LC.CASES[name]["T"]
    x = torch.from_numpy(LC.inputs(name, 0))
    out = []
    for dev in ("cpu", DEV):
        net = LC.build(_ns(), name).to(dev)
        mon = Monitor(net.connections[("X", "Y")], ["w"], time=T)
        net.add_monitor(mon, "w")
        net.run({"X": x.to(dev)}, time=T)
        out.append(mon.get("w").cpu().numpy())
    assert out[0].shape == (T, 2, 3 * 9, 12)
    assert np.array_equal(_bits(out[0]), _bits(out[1]))
    assert not np.array_equal(out[1][0], out[1][-1])          # the monitor sees the weights move


@pytest.mark.parametrize("mode", [0, 1])
def test_adaptive_lif_behind_connection_on_every_plan(mode):
    from bindsnet_amd import _lib
    L = _lib.lib()
    L.snn_set_plan_mode(mode)
    try:
        net, snaps = _run_device("f")
        plan = net.last_plan
    finally:
        L.snn_set_plan_mode(0)
    if mode == 1:
        assert plan == "generic"
    check_snapshots("f", snaps)


# ---- kernel sweeps: device vs the reference's torch expressions on the host -----------------------------------------------
def _lc(Cin, shape, k, s, F, B, wmin=None, wmax=None, nu=(0.0, 0.0), weight_decay=0.0, seed=0):
    from bindsnet_amd.learning.learning import PostPre
    from bindsnet_amd.network.nodes import AdaptiveLIFNodes, Input
    from bindsnet_amd.network.topology import LocalConnection1D, LocalConnection2D
    torch.manual_seed(seed)
    ks = k if isinstance(k, tuple) else (k,) * len(shape)
    ss = s if isinstance(s, tuple) else (s,) * len(shape)
    conv = [int((n - kk) / st) + 1 for n, kk, st in zip(shape, ks, ss)]
    X = Input(shape=[Cin, *shape], traces=True)
    Y = AdaptiveLIFNodes(shape=[F, int(np.prod(conv))] if len(shape) == 1 else [F, *conv], traces=True)
    kw = {} if wmin is None else {"wmin": wmin}
    if wmax is not None:
        kw["wmax"] = wmax
    cls = LocalConnection1D if len(shape) == 1 else LocalConnection2D
    c = cls(X, Y, kernel_size=k, stride=s, n_filters=F, nu=nu, update_rule=PostPre, weight_decay=weight_decay,
            reduction=torch.squeeze if B == 1 else torch.sum, **kw)
    X.set_batch_size(B)
    Y.set_batch_size(B)
    c.w.data = (c.w.data - 0.3) * 2.0                  # signed weights: exercises the sums' sign handling
    return c


def _spikes(B, n, density, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, n, generator=g) < density).to(torch.uint8)


PROP_SHAPES = [(kp, Cin, B, d) for kp in (1, 7, 144, 300, 1000) for Cin in (1, 2, 4) for B in (1, 3, 33)
               for d in (0.0, 0.01, 0.3, 1.0)]


def _check_prop(c, B, density, seed):
    from bindsnet_amd import ops
    from bindsnet_amd.network import host_path
    s = _spikes(B, c.source.n, density, seed)
    want = host_path._propagate_local(c, s.view(B, *c.source.shape)).reshape(B, -1)
    out = torch.full((B, c.target.n), float("nan"), device=DEV)
    ops.prop_local(c.w.data.to(DEV), c.src.to(DEV), s.to(DEV), out, c.n_filters)
    got = out.cpu()
    assert np.array_equal(_bits(got.numpy()), _bits(want.numpy())), \
        f"prop_local differs at {np.flatnonzero(_bits(got.numpy()) != _bits(want.numpy()))[:5]}"
    acc = out.clone()                                   # accumulate = 1: out + r
    ops.prop_local(c.w.data.to(DEV), c.src.to(DEV), s.to(DEV), acc, c.n_filters, accumulate=True)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits((want + want).numpy()))


@pytest.mark.parametrize("kp,Cin,B,density", PROP_SHAPES)
def test_prop_local_sweep(kp, Cin, B, density):
    c = _lc(Cin, (kp,), kp, 1, 3, B, seed=kp + Cin)      # conv_prod = 1: the kernel covers the input
    _check_prop(c, B, density, seed=kp * 7 + B)


@pytest.mark.parametrize("Cin,shape,k,s,F,B,density", [
    (2, (9, 11), (4, 3), (2, 3), 5, 3, 0.3),            # non-square 2D, stride pair
    (1, (20, 20), 12, 4, 50, 2, 0.05),                  # the loc2d geometry: R = 450 > 256 threads
    (1, (40000,), 4, 4, 1, 2, 0.01),                    # n_src = 40 000 > 32 KiB of staged spikes: global-memory form
    (1, (300000,), 1, 1, 1, 1, 0.01),                   # R = 300 000 > 1024 workgroups x 256 threads: stride loop
    (3, (16,), 5, 2, 300, 1, 0.3),                      # Cin 3, R = 1800
])
def test_prop_local_geometries(Cin, shape, k, s, F, B, density):
    c = _lc(Cin, shape, k, s, F, B)
    _check_prop(c, B, density, seed=F + B)


def _check_postpre(c, B, density, seed):
    from bindsnet_amd import ops
    from bindsnet_amd.network import host_path
    rule = c.update_rule
    g = torch.Generator().manual_seed(seed)
    c.source.s = _spikes(B, c.source.n, density, seed).bool().view(B, *c.source.shape)
    c.target.s = _spikes(B, c.target.n, density, seed + 1).bool().view(B, *c.target.shape)
    c.source.x = torch.rand(B, *c.source.shape, generator=g) * c.source.s
    c.target.x = torch.rand(B, *c.target.shape, generator=g) * (torch.rand(B, *c.target.shape, generator=g) < 0.5)
    w0 = c.w.data.clone()
    lo, hi = rule._bounds()
    W = w0.to(DEV)
    ops.local_postpre(W, c.src.to(DEV), c.source.s.reshape(B, -1).to(DEV).to(torch.uint8), c.source.x.reshape(B, -1).to(DEV),
                      c.target.s.reshape(B, -1).to(DEV).to(torch.uint8), c.target.x.reshape(B, -1).to(DEV), float(rule.nu[0]),
                      float(rule.nu[1]), c.n_filters, decay=float(rule.weight_decay), wmin=lo, wmax=hi)
    host_path._update_local(c, rule)
    got, want = _bits(W.cpu().numpy()).reshape(-1), _bits(c.w.data.numpy()).reshape(-1)
    assert np.array_equal(got, want), f"local_postpre differs at {np.flatnonzero(got != want)[:5]}"


POSTPRE_SHAPES = [(kp, Cin, B, d, v) for kp in (1, 7, 144, 300, 1000) for Cin in (1, 2, 4) for B in (1, 3, 33)
                  for d in (0.0, 0.01, 0.3, 1.0) for v in range(1)]
VARIANTS = [dict(nu=(1e-2, 2e-2)), dict(nu=(0.0, 3e-2), wmin=-0.5, wmax=0.7), dict(nu=(5e-2, 0.0), wmin=-0.1),
            dict(nu=(1e-2, 1e-2), wmax=0.4, weight_decay=0.01)]


@pytest.mark.parametrize("kp,Cin,B,density,v", POSTPRE_SHAPES)
def test_local_postpre_sweep(kp, Cin, B, density, v):
    variant = VARIANTS[(kp + Cin + B + int(density * 100)) % len(VARIANTS)]
    c = _lc(Cin, (kp,), kp, 1, 3, B, seed=kp + Cin, **variant)
    _check_postpre(c, B, density, seed=kp * 11 + B)


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("Cin,shape,k,s,F,B", [
    (2, (9, 11), (4, 3), (2, 3), 5, 3),                 # pins the raw [Cin, F*conv_prod, kernel_prod] reinterpretation
    (4, (1000,), 1000, 1, 300, 2),                      # 1.2 M weights > 4096 workgroups x 256 threads
    (1, (20, 20), (12, 12), (4, 4), 50, 33),            # the loc2d geometry at B = 33
    (3, (16,), 5, 2, 7, 3),
    (1, (1,), 1, 1, 1, 33),                             # one weight: ATen reduces the batch as an inner sum
    (1, (5,), 5, 1, 1, 33),                             # 4 <= numel < 8: four cascade columns, then row_sum
])
def test_local_postpre_geometries(variant, Cin, shape, k, s, F, B):
    c = _lc(Cin, shape, k, s, F, B, seed=F + variant, **VARIANTS[variant])
    _check_postpre(c, B, 0.3, seed=B + variant)


def test_unsupported_rules_raise_and_generic_plan_only():
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network.nodes import AdaptiveLIFNodes, Input
    from bindsnet_amd.network.topology import LocalConnection2D
    for rule in (learning.Hebbian, learning.WeightDependentPostPre, learning.MSTDP, learning.MSTDPET):
        with pytest.raises(NotImplementedError, match=f"{rule.__name__} on LocalConnection2D"):
            LocalConnection2D(Input(shape=[1, 8, 8], traces=True), AdaptiveLIFNodes(shape=[2, 3, 3], traces=True), kernel_size=4,
                              stride=2, n_filters=2, nu=0.1, update_rule=rule)
    net = LC.build(_ns(), "a").to(DEV)
    with pytest.raises(NotImplementedError, match="masks"):
        net.run({"X": torch.zeros(4, 1, 1, 20, 20, dtype=torch.uint8, device=DEV)}, time=4,
                masks={("X", "Y"): torch.zeros(1, 450, 144, dtype=torch.bool)})
    net2 = copy.deepcopy(LC.build(_ns(), "d")).to(DEV)
    net2.run({"X": torch.zeros(3, 1, 1, 6, 6, 6, dtype=torch.uint8, device=DEV)}, time=3)
    assert net2.last_plan == "generic"
