"""Hebbian / WeightDependentPostPre on a Conv2dConnection on the device: the per-operator entry snn_conv2d_hebbian, the generic plan that
calls it every timestep, and the one-launch plan `convpp-fused` whose apply step switches over the three outer-product rules.

  * every fixture recorded from the unmodified reference (OH*OW <= 64: tests/conv2d_rule_cases.py) on both plans, bit for bit;
  * fused == generic on the geometries of test_gpu_convpp.CASES that stress the fused kernel's limits, and with each chunk size forced;
  * the operator, and a whole run of the generic plan, against the order-pinned oracle helper (tests/conv_rule_oracle_run.py) at sizes
    where the reference's BLAS order is no longer the pinned one."""
import functools

import numpy as np
import pytest
import torch

import conv2d_rule_cases as CC
import synth
from conv_rule_oracle_run import ConvRuleOracleRun, apply_rule, conv_sums
from test_gpu_convpp import CASES as PP_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
u8, f32 = np.uint8, np.float32
RULES = ("Hebbian", "WeightDependentPostPre")
GEOMETRIES = ("conv_mnist_shape_b16", "stride2_pad1_b3", "two_input_channels_odd_cout", "multivalued_spike_bytes", "weight_decay_b17",
              "b33_tail_elements", "learning_off")


def _plan_mode(mode):
    from bindsnet_amd import _lib
    _lib.lib().snn_set_plan_mode(mode)


# ------------------------------------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize("mode,plan", [(0, "convpp-fused"), (1, "generic")])
@pytest.mark.parametrize("name", list(CC.CASES))
def test_device_plans_reproduce_the_reference_fixture(name, mode, plan):
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network, nodes, topology
    from bindsnet_amd.network.monitors import Monitor
    _plan_mode(mode)
    try:
        net = CC.build(CC.ns_from(nodes, topology, learning, Network), name)
        net.to(DEV)
        snaps = CC.run_case(net, name, Monitor, device=DEV)
        assert net.last_plan == plan
    finally:
        _plan_mode(0)
    CC.check_against_gold(snaps, name)


# ------------------------------------------------------------------------------------------------ fused == generic
def _bounds(rule, wmin, wmax):
    """WeightDependentPostPre needs both bounds: the case's own where it has them."""
    if rule == "WeightDependentPostPre":
        return (-0.2 if wmin is None else wmin), (0.9 if wmax is None else wmax)
    return wmin, wmax


def _build(rule, case):
    from bindsnet_amd import learning
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Conv2dConnection
    B, T, Cin, H, W, Cout, k, stride, pad, dens, vmax, nu, wmin, wmax, wd, vmon, learn = case
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    net = Network(dt=1.0, batch_size=B, learning=learn)
    net.add_layer(Input(shape=(Cin, H, W), traces=True), "X")
    net.add_layer(LIFNodes(shape=(Cout, OH, OW), traces=True), "Y")
    kw = dict(kernel_size=k, stride=stride, padding=pad, w=torch.from_numpy(synth.uniform_f32(7, (Cout, Cin, k, k), -0.1, 0.5)),
              update_rule=getattr(learning, rule), nu=nu, weight_decay=wd, reduction=torch.sum)
    lo, hi = _bounds(rule, wmin, wmax)
    if lo is not None:
        kw["wmin"] = lo
    if hi is not None:
        kw["wmax"] = hi
    net.add_connection(Conv2dConnection(net.layers["X"], net.layers["Y"], **kw), "X", "Y")
    return net


def _spikes(case, r):
    B, T, Cin, H, W = case[:5]
    dens, vmax = case[9], case[10]
    sp = synth.dense_spikes(60 + r, (T, B, Cin, H, W), dens)
    if vmax > 1:
        sp = (sp * np.random.RandomState(3 + r).randint(1, vmax + 1, size=sp.shape)).astype(u8)
    return sp


def run(mode, rule, case, n_runs=2):
    from bindsnet_amd.network.monitors import Monitor
    T, vmon = case[1], case[15]
    _plan_mode(mode)
    try:
        net = _build(rule, case)
        mons = {"s": Monitor(net.layers["Y"], ["s"], time=T)}
        if vmon:
            mons["v"] = Monitor(net.layers["Y"], ["v"], time=T)
        for n_, m in mons.items():
            net.add_monitor(m, n_)
        net.to(DEV)
        out = []
        w_start = net.connections[("X", "Y")].w.detach().cpu().numpy().copy()      # (after the constructor's clamp to the bounds)
        for r in range(n_runs):
            net.run({"X": torch.from_numpy(_spikes(case, r)).to(DEV)}, time=T)
            Y = net.layers["Y"]
            st = dict(s=mons["s"].get("s").cpu().numpy().copy(), v=Y.v.cpu().numpy().copy(), r=Y.refrac_count.cpu().numpy().copy(),
                      sl=Y.s.cpu().numpy().copy(), xY=Y.x.cpu().numpy().copy(), xX=net.layers["X"].x.cpu().numpy().copy(),
                      w=net.connections[("X", "Y")].w.detach().cpu().numpy().copy())
            if vmon:
                st["vm"] = mons["v"].get("v").cpu().numpy().copy()
            out.append(st)
        out[0]["w_start"] = w_start
        return out, net.last_plan
    finally:
        _plan_mode(0)


@functools.lru_cache(maxsize=None)
def generic(rule, name):
    """The per-operator plan's result, computed once and shared (read-only) by the tests below."""
    out, plan = run(1, rule, PP_CASES[name])
    assert plan == "generic"
    return out


def _same(a_runs, b_runs, what):
    for r, (a, b) in enumerate(zip(a_runs, b_runs)):
        for k in a:
            np.testing.assert_array_equal(a[k].view(u8), b[k].view(u8), err_msg=f"{what} run {r}: {k}")


def _not_vacuous(runs, case):
    assert sum(int(x["s"].sum()) for x in runs) > 0, "no output spike: vacuous"
    moved = not np.array_equal(runs[-1]["w"], runs[0]["w_start"])
    assert moved == bool(case[-1]), "the weights moved with learning off" if moved else "the weights never moved: vacuous"


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", GEOMETRIES)
def test_fused_equals_generic(name, rule):
    fused, plan = run(0, rule, PP_CASES[name])
    assert plan == "convpp-fused"
    _same(fused, generic(rule, name), f"{rule} {name}")
    _not_vacuous(fused, PP_CASES[name])


@pytest.mark.parametrize("cc", [2, 4, 8])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", ["conv_mnist_shape_b16", "two_input_channels_odd_cout"])
def test_every_chunk_size_of_the_fused_plan_equals_generic(name, rule, cc, monkeypatch):
    monkeypatch.setenv("SNN_CONVPP_CC", str(cc))
    fused, plan = run(0, rule, PP_CASES[name])
    assert plan == "convpp-fused"
    _same(fused, generic(rule, name), f"{rule} {name} cc {cc}")
    _not_vacuous(fused, PP_CASES[name])


# ------------------------------------------------------------------------------------------------ against the order-pinned oracle
#           (B, Cin, H, W, Cout, k, stride, pad)
OP_SHAPES = {
    "conv_mnist_b16": (16, 1, 28, 28, 32, 5, 1, 0),              # packed-row partial sums (k_conv_pp_partial_ev)
    "row_wider_than_32": (3, 2, 9, 40, 3, 3, 2, 1),              # the dense partial kernel (k_conv_pp_partial)
}


@functools.lru_cache(maxsize=None)
def _op_operands(shape_name):
    B, Cin, H, W, Cout, k, stride, pad = OP_SHAPES[shape_name]
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ops = dict(W0=synth.uniform_f32(2200, (Cout, Cin, k, k), -0.1, 0.5), s_src=synth.dense_spikes(2201, (B, Cin, H, W), 0.15),
               x_src=synth.uniform_f32(2202, (B, Cin, H, W), 0.0, 1.0), s_tgt=synth.dense_spikes(2203, (B, Cout, OH, OW), 0.1),
               x_tgt=synth.uniform_f32(2204, (B, Cout, OH, OW), 0.0, 1.0))
    ops["pre"], ops["post"] = conv_sums(ops["W0"].shape, ops["s_src"], ops["x_src"], ops["s_tgt"], ops["x_tgt"], stride, pad)
    for a in ops.values():
        a.setflags(write=False)
    return ops


# (rates sized for sums over up to 16 x 576 terms: the updates stay inside the bounds for most elements, so the clamp does not hide them)
@pytest.mark.parametrize("rule,kw", [("Hebbian", dict(nu=(1e-3, 1e-2))), ("Hebbian", dict(nu=(0.0, 1e-4), weight_decay=0.01, wmax=0.45)),
                                     ("WeightDependentPostPre", dict(nu=(2e-4, 1e-4), wmin=-0.2, wmax=0.7)),
                                     ("WeightDependentPostPre", dict(nu=(2e-4, 0.0), wmin=-0.2, wmax=0.7, weight_decay=0.02))])
@pytest.mark.parametrize("shape_name", list(OP_SHAPES))
def test_operator_equals_the_order_pinned_oracle(shape_name, rule, kw):
    """A hand-stepped connection.update() (ops.conv2d_hebbian -> snn_conv2d_hebbian) on prepared layer state."""
    from bindsnet_amd import learning
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Conv2dConnection
    B, Cin, H, W, Cout, k, stride, pad = OP_SHAPES[shape_name]
    o = _op_operands(shape_name)
    OH, OW = o["s_tgt"].shape[2:]
    src, tgt = Input(shape=(Cin, H, W), traces=True), LIFNodes(shape=(Cout, OH, OW), traces=True)
    c = Conv2dConnection(src, tgt, kernel_size=k, stride=stride, padding=pad, w=torch.from_numpy(o["W0"].copy()), update_rule=getattr(learning, rule),
                         reduction=torch.sum, **kw).to(DEV)
    for l, s, x in ((src, o["s_src"], o["x_src"]), (tgt, o["s_tgt"], o["x_tgt"])):
        l.batch_size = B
        l.s, l.x = torch.from_numpy(s.copy()).to(DEV), torch.from_numpy(x.copy()).to(DEV)
    start = c.w.detach().cpu().numpy().copy()            # (the constructor clamps the given weights to the bounds)
    want = start.copy()
    c.update(learning=True)
    apply_rule(want, o["pre"], o["post"], weight_dependent=rule == "WeightDependentPostPre", nu0=kw["nu"][0], nu1=kw["nu"][1],
               decay=c.update_rule.weight_decay, wmin=kw.get("wmin"), wmax=kw.get("wmax"))
    got = c.w.detach().cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert int(o["s_tgt"].sum()) > 0 and int(o["s_src"].sum()) > 0 and not np.array_equal(got, start), "vacuous"
    assert np.unique(want).size > want.size // 2, "most elements sit at a bound: the clamp hides the update"


@pytest.mark.parametrize("rule", RULES)
def test_generic_plan_run_equals_the_order_pinned_oracle_beyond_64_positions(rule):
    """OH*OW = 144: past the sizes at which the reference's bmm keeps the ascending order, the pinned order is the oracle's."""
    case = (3, 25, 1, 16, 16, 6, 5, 1, 0, 0.3, 1, (1e-3, 1e-2), None, 0.8, 0.01, False, True)
    oracle_run = ConvRuleOracleRun(_build(rule, case), case[0])
    _plan_mode(1)
    try:
        net = _build(rule, case)
        from bindsnet_amd.network.monitors import Monitor
        mon = Monitor(net.layers["Y"], ["s"], time=case[1])
        net.add_monitor(mon, "s")
        net.to(DEV)
        for r in range(2):
            sp = _spikes(case, r)
            want = oracle_run.run(sp)
            net.run({"X": torch.from_numpy(sp).to(DEV)}, time=case[1])
            assert net.last_plan == "generic"
            Y = net.layers["Y"]
            got = dict(s=mon.get("s").cpu().numpy().astype(u8).reshape(want["s"].shape), v=Y.v.cpu().numpy(), refrac_count=Y.refrac_count.cpu().numpy(),
                       xY=Y.x.cpu().numpy(), xX=net.layers["X"].x.cpu().numpy(), W=net.connections[("X", "Y")].w.detach().cpu().numpy())
            for k, a in got.items():
                np.testing.assert_array_equal(np.ascontiguousarray(a).view(u8), np.ascontiguousarray(want[k]).view(u8), err_msg=f"run {r}: {k}")
        assert int(want["s"].sum()) > 0 and not np.array_equal(got["W"], synth.uniform_f32(7, got["W"].shape, -0.1, 0.5)), "vacuous"
    finally:
        _plan_mode(0)


def test_weight_dependent_without_both_bounds_is_an_invalid_argument():
    from bindsnet_amd import _lib
    L = _lib.lib()
    B, Cin, H, W, Cout, k = 2, 1, 8, 8, 3, 3
    Wt = torch.full((Cout, Cin, k, k), 0.25, device=DEV)
    s_src, x_src = torch.ones(B, Cin, H, W, dtype=torch.uint8, device=DEV), torch.ones(B, Cin, H, W, device=DEV)
    s_tgt, x_tgt = torch.ones(B, Cout, 6, 6, dtype=torch.uint8, device=DEV), torch.ones(B, Cout, 6, 6, device=DEV)
    ws = torch.zeros(2 * B * Wt.numel(), device=DEV)
    p = lambda t: t.data_ptr()      # noqa: E731
    for has_min, has_max in ((0, 0), (1, 0), (0, 1)):
        rc = L.snn_conv2d_hebbian(p(Wt), p(s_src), p(x_src), p(s_tgt), p(x_tgt), B, Cin, H, W, Cout, k, k, 1, 0, 1e-3, 1e-2, 1, 1.0,
                                  has_min, 0.0, has_max, 1.0, p(ws), None)
        assert rc == -1                       # SNN_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(Wt, torch.full_like(Wt, 0.25)), "a refused call must not touch the weights"
    assert L.snn_conv2d_hebbian(p(Wt), p(s_src), p(x_src), p(s_tgt), p(x_tgt), B, Cin, H, W, Cout, k, k, 1, 0, 1e-3, 1e-2, 1, 1.0,
                                1, 0.0, 1, 1.0, p(ws), None) == 0
    torch.cuda.synchronize()
    assert not torch.equal(Wt, torch.full_like(Wt, 0.25))


@pytest.mark.parametrize("mode,plan", [(0, "convpp-fused"), (1, "generic")])
def test_hebbian_with_a_zero_rate_still_adds_and_turns_negative_zero_into_positive_zero(mode, plan):
    """learning.py:1374 / :1378 run whatever the rates are: `w += 0 * post` rewrites a -0.0 weight as +0.0 -- in both apply kernels."""
    from bindsnet_amd.learning import Hebbian
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Conv2dConnection
    _plan_mode(mode)
    try:
        X, Y = Input(shape=[1, 6, 6], traces=True), LIFNodes(shape=[4, 4, 4], traces=True)
        w = torch.full((4, 1, 3, 3), -0.0)
        w[0] = 5.0                                   # one channel that spikes
        net = Network(dt=1.0)
        net.add_layer(X, "X")
        net.add_layer(Y, "Y")
        net.add_connection(Conv2dConnection(X, Y, kernel_size=3, update_rule=Hebbian, nu=(1e-3, 0.0), w=w), "X", "Y")
        net.to(DEV)
        assert np.signbit(net.connections[("X", "Y")].w.cpu().numpy()[1:]).all()
        net.run({"X": torch.ones(3, 1, 1, 6, 6, dtype=torch.uint8, device=DEV)}, time=3)
        assert net.last_plan == plan
        got = net.connections[("X", "Y")].w.cpu().numpy()
        assert (got[1:] == 0).all() and not np.signbit(got[1:]).any()
        assert not np.array_equal(got[0], np.full((1, 3, 3), 5.0, f32)), "the spiking channel never learned: vacuous"
    finally:
        _plan_mode(0)
