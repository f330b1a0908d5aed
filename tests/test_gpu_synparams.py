"""Per-synapse learning rates, weight bounds and per-target norms on the device (the *_pv entry points of include/snnhip.h f13 and
the generic plan of snn_net_run that uses them):

  * every fixture case of tests/synparams_cases.py (written by the unmodified reference): the op-level cases and the
    MulticompartmentConnection runs bit for bit, the dense Connection runs raster-equal with weights within 1e-5, all on the generic
    plan; the same graphs with scalar constants keep the plan they have without this feature;
  * the device against the kernels' own bodies on the host (tests/synparams_hostlib.py) on shapes around every limit of the launch
    code: 16-row x TJ-column tiles whose TJ falls from 256 to 32 as the batch grows (LDS), grids capped at 4096 workgroups of 256
    threads (k_mstdpet_pv, k_scale_cols), S = 1, N = 1, B = 1 .. 256, every constant in every shape that broadcasts against [S, N];
  * two half runs equal one whole run; an in-place edit of conn.wmax between runs takes effect; a weight Monitor agrees step by
    step with the host path; the device raises what the host path raises."""
import builtins
import warnings

import numpy as np
import pytest
import torch

import synparams_cases as SC
from test_synparams_host import RAISES, bits, check_op, check_run, ns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


@pytest.mark.parametrize("case", list(SC.OP_CASES))
def test_op_cases_bit_for_bit(case):
    net, conn = _quiet(SC.build_op, ns(), case)
    net.to(DEV)
    host_only_norm = SC.VARIANTS[SC.OP_CASES[case]["variant"]]["norm"] == "SN"
    got = SC.run_op(net, conn, case, device=DEV, normalize=not host_only_norm)
    check_op(case, got, skip=("w_norm",) if host_only_norm else ())
    if host_only_norm:
        with pytest.raises(NotImplementedError, match="one entry per target neuron"):
            conn.normalize()


@pytest.mark.parametrize("case", list(SC.RUN_CASES))
def test_run_cases_on_the_generic_plan(case):
    n = ns()
    net = SC.build_run(n, case)
    net.to(DEV)
    got = SC.run_run(n, net, case, device=DEV)
    assert net.last_plan == "generic"
    check_run(case, got, exact=SC.RUN_CASES[case]["kind"] == "mcc")


# the plans the same graphs take with scalar constants (every tensor replaced by its mean), as before per-synapse constants existed
SCALAR_PLANS = {"mcc_postpre": "generic", "mcc_mstdp": "generic", "dense_postpre": "generic", "dense_hebbian": "generic"}


@pytest.mark.parametrize("case", list(SC.RUN_CASES))
def test_scalar_graphs_keep_their_plan(case):
    n = ns()
    net = SC.build_run(n, case, "mean")
    net.to(DEV)
    SC.run_run(n, net, case, device=DEV, n_in=1)
    print("plan", case, net.last_plan)
    assert net.last_plan == SCALAR_PLANS[case]


def test_a_fused_scalar_graph_keeps_its_plan_and_tensors_take_the_generic_one():
    """tools/bench_synparams.py's dense graph (Input 784 -> Connection + PostPre -> LIF 400, B = 16) without the tool's plan switch:
    with scalars it is a dense-family graph of the one-launch plan; any tensor constant sends it to the generic plan."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_synparams.py")
    spec = importlib.util.spec_from_file_location("bench_synparams", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    x = (torch.rand(20, 16, tool.S, device=DEV) < 0.1).to(torch.uint8)
    for mode, plan in (("scalar", "twolayer-fused"), ("uniform", "generic"), ("tensor", "generic")):
        net = tool.build("dense", mode)
        net.run({"X": x}, time=20)
        assert net.last_plan == plan, (mode, net.last_plan)


def _extra_net(n, rule, B, seed):
    """Input 40 -> Connection (rule; [S, N] rates, [S, 1] / [1, N] bounds, [N] norm) -> LIF 30: the rules no run-level fixture has."""
    rng = np.random.default_rng(seed)
    S, N = SC.R_S, SC.R_N
    draw = lambda shape, lo, hi: torch.from_numpy((lo + (hi - lo) * rng.random(shape)).astype(np.float32))      # noqa: E731
    lo, hi = {"WeightDependentPostPre": (0.01, 0.05), "MSTDP": (0.01, 0.05), "MSTDPET": (0.05, 0.3)}[rule]
    net = n.Network(dt=1.0, batch_size=B)
    X = n.Input(n=S, traces=True, tc_trace=20.0)
    Y = n.LIFNodes(n=N, traces=True, tc_trace=20.0, thresh=-52.0, rest=-65.0, reset=-65.0, refrac=5, tc_decay=100.0)
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    conn = n.Connection(X, Y, w=draw((S, N), 0.25, 0.55), wmin=draw((S, 1), 0.1, 0.3), wmax=draw((1, N), 0.5, 0.7), norm=draw((N,), 12.0, 18.0),
                        update_rule=getattr(n.learning, rule), nu=[draw((S, N), lo, hi), draw((S, N), lo, hi)],
                        reduction=torch.sum if B > 1 else None)
    net.add_connection(conn, source="X", target="Y")
    return net


@pytest.mark.parametrize("rule,B", [("WeightDependentPostPre", 3), ("MSTDP", 3), ("MSTDPET", 1)])
def test_net_run_agrees_with_the_host_path_on_the_other_rules(rule, B):
    """snn_net_run's dispatch to snn_stdp_hebbian_pv (weight-dependent), snn_mstdp_step_pv with a tensor nu[0] and
    snn_mstdpet_step_pv, descriptors included: two runs against the host path -- equal rasters, weights within the dense family's 1e-5."""
    n = ns()
    outs = []
    for dev in (None, DEV):
        net = _quiet(_extra_net, n, rule, B, 50 + B)
        if dev:
            net.to(dev)
        mon = n.Monitor(net.layers["Y"], ["s"], time=2 * SC.R_T)
        net.add_monitor(mon, name="Y_mon")
        ws = []
        for r in range(2):
            x = torch.from_numpy((np.random.default_rng(60 + r).random((SC.R_T, B, SC.R_S)) < 0.25).astype(np.uint8))
            net.run({"X": x.to(dev) if dev else x}, time=SC.R_T, reward=0.7 if r == 0 else -0.4)
            ws.append(net.connections[("X", "Y")].w.detach().cpu().numpy().copy())
        if dev:
            assert net.last_plan == "generic"
        outs.append((mon.get("s").cpu().numpy().astype(np.uint8), ws))
    assert outs[0][0].sum() >= 50 and np.array_equal(outs[0][0], outs[1][0])
    assert not np.array_equal(outs[1][1][0], outs[1][1][1])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert np.abs(a - b).max() <= 1e-5, np.abs(a - b).max()


def test_mcc_range_of_a_float_and_a_tensor_equals_the_host_path():
    n = ns()
    outs = []
    for dev in (None, DEV):
        net = SC.build_run(n, "mcc_postpre")
        net.connections[("X", "Y")].pipeline[0].learning_rule.min = 0.2
        if dev:
            net.to(dev)
        outs.append(SC.run_run(n, net, "mcc_postpre", device=dev, n_in=1)[0])
    assert np.array_equal(outs[0]["raster"], outs[1]["raster"]) and np.array_equal(bits(outs[0]["w"]), bits(outs[1]["w"]))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    from synparams_hostlib import HostLib
    return HostLib(tmp_path_factory.mktemp("hostcheck"))


SHAPES = ("SN", "N", "1N", "S1", "1", "float")


def _const(rng, code, S, N, lo, hi):
    if code == "float":
        return float(np.float32(lo + (hi - lo) * rng.random()))
    shape = {"SN": (S, N), "N": (N,), "1N": (1, N), "S1": (S, 1), "1": (1,)}[code]
    return torch.from_numpy((lo + (hi - lo) * rng.random(shape)).astype(np.float32))


# (S, N, B): S * N no multiple of 256 and of a tile; several tiles each way; one row; one column; the TJ = 128 / 64 / 32 tiles
SWEEP = ((37, 29, 1), (37, 29, 33), (1, 300, 3), (300, 1, 3), (70, 530, 2), (20, 140, 64), (20, 70, 130), (18, 40, 256))


@pytest.mark.parametrize("mode", ["postpre", "hebbian", "wdpostpre", "mstdp"])
def test_update_entry_points_equal_the_host_bodies(host, mode):
    from bindsnet_amd import ops
    rng = np.random.default_rng(10 + len(mode))
    k = 0
    for S, N, B in SWEEP:
        for rep in range(6 if S * N < 5000 else 2):
            a, b, c = SHAPES[k % 6], SHAPES[(k // 2 + 1) % 6], SHAPES[(k // 3 + 3) % 6]
            k += 1
            if mode == "postpre" and a in ("SN", "S1"):
                a = "N"
            nu0, nu1 = _const(rng, a, S, N, -0.3, 0.3), _const(rng, a, S, N, 0.0, 0.3)
            wmin, wmax = _const(rng, b, S, N, 0.1, 0.4), _const(rng, c, S, N, 0.6, 0.9)
            W = torch.from_numpy(rng.random((S, N)).astype(np.float32))
            ss, st = torch.from_numpy(rng.random((B, S)) < 0.3), torch.from_numpy(rng.random((B, N)) < 0.3)
            xs, xt = torch.from_numpy(rng.random((B, S)).astype(np.float32)), torch.from_numpy(rng.random((B, N)).astype(np.float32))
            want = W.clone()
            host.update(mode, want, ss, xs, st, xt, nu0, nu1, use_dt=mode == "postpre", dt=0.5, decay=0.99, wmin=wmin, wmax=wmax, reward=0.7)
            Wd, d = W.to(DEV), (lambda t: t.to(DEV).contiguous())
            if mode == "postpre":
                ops.stdp_postpre(Wd, d(ss), d(xs), d(st), d(xt), nu0, nu1, use_dt=True, dt=0.5, decay=0.99, wmin=wmin, wmax=wmax)
            elif mode == "mstdp":
                pp, pm, sp, tp = d(xs), d(xt), d(ss).to(torch.uint8), d(st).to(torch.uint8)
                ops.mstdp_step(Wd, pp, pm, sp, tp, d(ss), d(st), 0.7, nu0, 1.0, -1.0, 0.9, 0.9, wdecay=0.99, wmin=wmin, wmax=wmax)
            else:
                ops.stdp_hebbian(Wd, d(ss), d(xs), d(st), d(xt), nu0, nu1, weight_dependent=mode == "wdpostpre", decay=0.99, wmin=wmin, wmax=wmax)
            got = Wd.cpu()
            assert np.array_equal(bits(got.numpy()), bits(want.numpy())), (mode, S, N, B, a, b, c, int((bits(got.numpy()) != bits(want.numpy())).sum()))


def test_postpre_skips_untouched_elements_only_where_it_may(host):
    """assume_clamped (what snn_net_run passes from the second step on): elements without a pre- or post-synaptic spike are not
    visited -- weights inside their own bounds come out as from the full pass."""
    from bindsnet_amd import ops
    rng = np.random.default_rng(3)
    S, N, B = 70, 530, 3
    wmin, wmax = _const(rng, "SN", S, N, 0.1, 0.4), _const(rng, "N", S, N, 0.6, 0.9)
    nu0, nu1 = _const(rng, "N", S, N, 0.0, 0.3), _const(rng, "1N", S, N, 0.0, 0.3)
    W = torch.clamp(torch.from_numpy(rng.random((S, N)).astype(np.float32)), wmin, wmax)
    ss, st = torch.from_numpy(rng.random((B, S)) < 0.05), torch.from_numpy(rng.random((B, N)) < 0.05)
    xs, xt = torch.from_numpy(rng.random((B, S)).astype(np.float32)), torch.from_numpy(rng.random((B, N)).astype(np.float32))
    want = W.clone()
    host.update("postpre", want, ss, xs, st, xt, nu0, nu1, wmin=wmin, wmax=wmax)
    Wd = W.to(DEV)
    ops.stdp_postpre(Wd, ss.to(DEV), xs.to(DEV), st.to(DEV), xt.to(DEV), nu0, nu1, use_dt=False, wmin=wmin, wmax=wmax, assume_clamped=True)
    assert np.array_equal(bits(Wd.cpu().numpy()), bits(want.numpy()))


def test_mstdpet_and_normalize_equal_the_host_bodies(host):
    from bindsnet_amd import ops
    rng = np.random.default_rng(21)
    for k, (S, N) in enumerate(((37, 29), (1, 300), (300, 1), (1030, 1021))):      # the last: more than 4096 x 256 elements, a second grid pass
        a, b, c = SHAPES[k % 6], SHAPES[(k + 2) % 6], SHAPES[(k + 3) % 6]
        nu0 = _const(rng, a, S, N, 0.5, 6.0)
        wmin, wmax = _const(rng, b, S, N, 0.1, 0.4), _const(rng, c, S, N, 0.6, 0.9)
        W = torch.from_numpy(rng.random((S, N)).astype(np.float32))
        et = torch.from_numpy((rng.random((S, N)) * 0.1).astype(np.float32))
        pp, pm = torch.from_numpy(rng.random(S).astype(np.float32)), torch.from_numpy(-rng.random(N).astype(np.float32))
        sp, tp = torch.from_numpy((rng.random(S) < 0.3).astype(np.uint8)), torch.from_numpy((rng.random(N) < 0.3).astype(np.uint8))
        want, want_e = W.clone(), et.clone()
        host.mstdpet(want, want_e, pp, pm, sp, tp, -0.75, nu0, 1.0, 0.96, 25.0, wdecay=0.99, wmin=wmin, wmax=wmax)
        Wd, ed = W.to(DEV), et.to(DEV)
        ops.mstdpet_step(Wd, ed, pp.to(DEV), pm.to(DEV), sp.to(DEV), tp.to(DEV), sp.to(DEV), tp.to(DEV), -0.75, nu0, 1.0, 1.0, -1.0, 0.9, 0.9,
                         0.96, 25.0, wdecay=0.99, wmin=wmin, wmax=wmax)
        assert np.array_equal(bits(Wd.cpu().numpy()), bits(want.numpy())), (S, N, a, b, c)
        assert np.array_equal(bits(ed.cpu().numpy()), bits(want_e.numpy())), (S, N)
        for use_abs in (True, False):          # weights that are multiples of 1/8: every column sum is exact, whatever its order
            norm = torch.from_numpy((1.0 + rng.random((N,) if k % 2 else (1, N)) * 20).astype(np.float32))
            V = torch.from_numpy((rng.integers(-3, 9, size=(S, N)) / 8.0).astype(np.float32))
            V[:, 0] = 0.0                       # the zero -> 1 guard
            want = V.clone()
            host.normalize(want, norm, use_abs)
            Vd = V.to(DEV)
            ops.normalize(Vd, norm, use_abs=use_abs)
            assert np.array_equal(bits(Vd.cpu().numpy()), bits(want.numpy())), (S, N, use_abs)


def test_two_half_runs_equal_one_whole_run():
    n = ns()
    for case in SC.RUN_CASES:
        nets = [SC.no_norm(SC.build_run(n, case)).to(DEV) for _ in range(2)]
        whole = SC.run_run(n, nets[0], case, device=DEV, n_in=1)
        halves = SC.run_run(n, nets[1], case, device=DEV, n_in=1, split=25)
        assert np.array_equal(whole[0]["raster"], halves[0]["raster"]), case
        assert np.array_equal(bits(whole[0]["w"]), bits(halves[0]["w"])), case


def test_an_edit_of_wmax_between_runs_takes_effect():
    n = ns()
    limit = float(np.float32(0.3))
    for edit in (lambda c: c.wmax.fill_(0.3),
                 lambda c: setattr(c, "wmax", torch.nn.Parameter(torch.full((SC.R_S, SC.R_N), 0.3, device=DEV), requires_grad=False))):
        net = SC.no_norm(SC.build_run(n, "dense_postpre")).to(DEV)
        conn = net.connections[("X", "Y")]
        SC.run_run(n, net, "dense_postpre", device=DEV, n_in=1)
        assert float(conn.w.max()) > limit
        edit(conn)
        SC.run_run(n, net, "dense_postpre", device=DEV, n_in=1)
        assert float(conn.w.max()) <= limit
    # ... and so do an edit of the rates and of the norm
    net = SC.build_run(n, "dense_postpre").to(DEV)
    conn = net.connections[("X", "Y")]
    SC.run_run(n, net, "dense_postpre", device=DEV, n_in=1)
    conn.update_rule.nu.zero_()
    conn.norm.fill_(5.0)
    before = conn.w.detach().clone()
    SC.run_run(n, net, "dense_postpre", device=DEV, n_in=1)
    clamped = torch.clamp(before, conn.wmin.detach(), conn.wmax.detach())       # (zero rates: the update is the clamp alone)
    assert torch.allclose(conn.w.detach(), clamped * (5.0 / clamped.abs().sum(0)), rtol=1e-5, atol=0)
    assert not torch.equal(clamped, before)


def test_weight_monitor_agrees_with_the_host_path():
    n = ns()
    runs = []
    for dev in (None, DEV):
        net = SC.build_run(n, "dense_postpre")
        if dev:
            net.to(dev)
        mon = n.Monitor(net.connections[("X", "Y")], ["w"], time=SC.R_T)
        net.add_monitor(mon, name="w_mon")
        out = SC.run_run(n, net, "dense_postpre", device=dev, n_in=1)
        runs.append((out[0]["raster"], mon.get("w").cpu().numpy().reshape(SC.R_T, SC.R_S, SC.R_N)))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.abs(runs[0][1] - runs[1][1]).max() <= 1e-5
    assert not np.array_equal(runs[1][1][0], runs[1][1][-1])


@pytest.mark.parametrize("name", list(SC.RAISES))
def test_the_device_raises_what_the_host_path_raises(name):
    with pytest.raises(getattr(builtins, RAISES[name]["type"])):
        _quiet(SC.raises_trial, ns(), name, device=DEV)


def test_wdpostpre_refuses_a_bound_made_non_finite_in_place():
    n = ns()
    from bindsnet_amd.learning import WeightDependentPostPre
    net = n.Network(dt=1.0)
    X, Y = n.Input(n=6, traces=True), n.LIFNodes(n=5, traces=True)
    conn = n.Connection(X, Y, w=torch.rand(6, 5), wmin=torch.zeros(6, 5), wmax=torch.ones(6, 5), update_rule=WeightDependentPostPre, nu=(0.1, 0.1))
    net.add_layer(X, name="X")
    net.add_layer(Y, name="Y")
    net.add_connection(conn, source="X", target="Y")
    net.to(DEV)
    x = (torch.rand(10, 1, 6, device=DEV) < 0.5).to(torch.uint8)
    net.run({"X": x}, time=10)
    assert net.last_plan == "generic"
    conn.wmax[2, 3] = float("inf")
    w = conn.w.detach().clone()
    with pytest.raises(NotImplementedError, match="finite wmin and wmax for every synapse"):
        net.run({"X": x}, time=10)
    assert torch.equal(conn.w.detach(), w)
