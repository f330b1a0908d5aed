"""Per-synapse learning rates, weight bounds and per-target norms on the package's host path (network/host_path.py) against the
fixtures the unmodified reference wrote (tests/golden/make_golden_synparams.py, cases in tests/synparams_cases.py):

  * every op-level case (K update() calls on set states, then normalize()) and the MulticompartmentConnection run-level cases bit for
    bit; the dense run-level cases raster-equal with weights within 1e-5 (the reference's matmul order is MKL's: README "Parity");
  * every entry of synparams_raises.json raises its recorded type and leaves the weights and the layer state untouched;
  * tensors filled with one value equal the scalar run bit for bit for rates and bounds on all five rules -- and do NOT for the
    norm, which a tensor divides by (norm / colsum) where a float multiplies by the reciprocal;
  * the refusals that stay: Rmax, half-precision Weights, the convolutional families, the multi-device modes;
  * Connection(wmin=tensor, wmax=tensor) without `w=` draws and clamps like topology.py:309-318; save / clone / to carry the constants."""
import io
import json
import os
import warnings

import numpy as np
import pytest
import torch

import synparams_cases as SC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def ns():
    from bindsnet_amd.learning import MCC_learning, learning
    from bindsnet_amd.network import Network, nodes, topology, topology_features
    from bindsnet_amd.network.monitors import Monitor
    return SC.ns_from(nodes, topology, topology_features, learning, MCC_learning, Network, Monitor)


_GOLD = {}


def gold(name):
    if name not in _GOLD:
        _GOLD[name] = np.load(os.path.join(GOLD, name))
    return _GOLD[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_op(case, got, skip=()):
    g = gold(f"synparams_op_{SC.OP_CASES[case]['rule']}.npz")
    keys = [k[len(case) + 1:] for k in g.files if k.startswith(case + "/")]
    assert keys and "w_norm" in keys
    for key in keys:
        if key in skip:
            continue
        want = g[f"{case}/{key}"]
        assert key in got, f"{case}: {key} missing"
        a = got[key].reshape(want.shape)
        assert np.array_equal(bits(a), bits(want)), f"{case}: {key} differs in {(bits(a) != bits(want)).sum()} of {want.size} elements"


@pytest.mark.parametrize("case", list(SC.OP_CASES))
def test_op_cases_bit_for_bit(case):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = SC.run_op(*SC.build_op(ns(), case), case)
    check_op(case, got)


@pytest.mark.parametrize("case", list(SC.OP_CASES))
def test_fixture_conditions_hold(case):
    """The generator's own conditions, re-asserted on the committed fixture (against this package's mean-constants run)."""
    g = gold(f"synparams_op_{SC.OP_CASES[case]['rule']}.npz")
    got = {k[len(case) + 1:]: g[k] for k in g.files if k.startswith(case + "/")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mean = SC.run_op(*SC.build_op(ns(), case, "mean"), case)
    SC.op_conditions(case, got, mean)


def check_run(case, got, exact):
    g = gold("synparams_run.npz")
    for r, out in enumerate(got):
        want = np.unpackbits(g[f"{case}/raster{r}"])[:out["raster"].size].reshape(out["raster"].shape)
        assert np.array_equal(out["raster"], want), f"{case} input {r}: {(out['raster'] != want).sum()} raster slots differ"
        for key in ("w", "v"):
            a, b = out[key], g[f"{case}/{key}{r}"].reshape(out[key].shape)
            if exact:
                assert np.array_equal(bits(a), bits(b)), f"{case} input {r}: {key} differs in {(bits(a) != bits(b)).sum()} elements"
            elif key == "w":
                assert np.abs(a - b).max() <= 1e-5, f"{case} input {r}: w differs by {np.abs(a - b).max()}"


@pytest.mark.parametrize("case", list(SC.RUN_CASES))
def test_run_cases(case):
    n = ns()
    got = SC.run_run(n, SC.build_run(n, case), case)
    check_run(case, got, exact=SC.RUN_CASES[case]["kind"] == "mcc")


@pytest.mark.parametrize("case", list(SC.RUN_CASES))
def test_run_fixture_conditions_hold(case):
    """The generator's conditions for the run-level cases, re-asserted on the committed fixture: spikes, w moves, both clamps bind
    on learned weights where the bounds differ, the mean-constants run differs, norm / colsum differs from norm * (1 / colsum)."""
    g = gold("synparams_run.npz")
    n = ns()
    got = [dict(raster=np.unpackbits(g[f"{case}/raster{r}"])[:SC.R_T * SC.R_B * SC.R_N].reshape(SC.R_T, SC.R_B, SC.R_N), w=g[f"{case}/w{r}"])
           for r in range(2)]
    mean = SC.run_run(n, SC.build_run(n, case, "mean"), case)
    SC.run_conditions(case, got, mean, *SC.pre_norm_weights(n, case))


def test_mcc_range_of_a_float_and_a_tensor_runs_like_two_tensors():
    """range=[float, tensor] is outside the reference's contract ([tensor, tensor]); both paths of this package run it, as the
    tensor pair with the float filled in."""
    n = ns()
    outs = []
    for fill in (False, True):
        net = SC.build_run(n, "mcc_postpre")
        rule = net.connections[("X", "Y")].pipeline[0].learning_rule
        rule.min = torch.full_like(rule.min, 0.2) if fill else 0.2
        outs.append(SC.run_run(n, net, "mcc_postpre", n_in=1)[0])
    assert np.array_equal(outs[0]["raster"], outs[1]["raster"]) and np.array_equal(bits(outs[0]["w"]), bits(outs[1]["w"]))


def test_two_half_runs_equal_one_whole_run():
    """(without a norm: run() normalises behind every call)"""
    n = ns()
    for case in SC.RUN_CASES:
        nets = [SC.no_norm(SC.build_run(n, case)) for _ in range(2)]
        whole = SC.run_run(n, nets[0], case, n_in=1)
        halves = SC.run_run(n, nets[1], case, n_in=1, split=25)
        assert np.array_equal(whole[0]["raster"], halves[0]["raster"]), case
        assert np.array_equal(bits(whole[0]["w"]), bits(halves[0]["w"])), case


RAISES = json.load(open(os.path.join(GOLD, "synparams_raises.json")))


@pytest.mark.parametrize("name", list(SC.RAISES))
def test_raises_what_the_reference_raises(name):
    import builtins
    want = RAISES[name]["type"]
    assert want != "ok"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(getattr(builtins, want)):
            SC.raises_trial(ns(), name)
    st = SC.raises_trial.last
    Y = st["Y"]
    assert float(Y.v.min()) == float(Y.v.max()) == float(Y.rest) and not Y.s.any(), "the layer state moved before the refusal"
    if "conn" in st:
        w = SC.run_weights(st["net"]) if st["net"].connections else st["w"]
        assert torch.equal(w.detach().cpu(), st["w"]), "the weights moved before the refusal"


@pytest.mark.parametrize("rule", SC.RULES)
def test_uniform_rates_and_bounds_equal_scalars_but_a_uniform_norm_divides(rule):
    cases = [c for c, d in SC.OP_CASES.items() if d["rule"] == rule]
    for case in cases:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            uni = SC.run_op(*SC.build_op(ns(), case, "uniform"), case)
            sca = SC.run_op(*SC.build_op(ns(), case, "mean"), case)
        for k in range(SC.K):
            assert np.array_equal(bits(uni[f"w{k}"]), bits(sca[f"w{k}"])), f"{case}: call {k}, uniform tensors differ from the scalars"
        pre = torch.from_numpy(uni[f"w{SC.K - 1}"])
        colsum = pre.abs().sum(0)
        norm = torch.from_numpy(np.asarray(SC.constants(case, "uniform")["norm"], np.float32))
        assert np.array_equal(bits(uni["w_norm"]), bits((pre * (norm / colsum.unsqueeze(0))).numpy())), case      # the fixture's expression ...
        recip = pre * (float(SC.constants(case, "mean")["norm"]) / colsum.unsqueeze(0))
        assert np.array_equal(bits(sca["w_norm"]), bits(recip.numpy())), case                                      # ... the scalar's
    differs = [c for c in cases if not np.array_equal(bits(SC.run_op(*SC.build_op(ns(), c, "uniform"), c)["w_norm"]),
                                                      bits(SC.run_op(*SC.build_op(ns(), c, "mean"), c)["w_norm"]))]
    assert differs, f"{rule}: a uniform norm tensor gives the scalar norm's weights in every case"


def test_wdpostpre_refuses_a_non_finite_bound():
    from bindsnet_amd.learning import WeightDependentPostPre
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Connection
    wmax = torch.full((4, 3), 1.0)
    wmax[1, 2] = float("inf")
    with pytest.raises(NotImplementedError, match="finite wmin and wmax for every synapse"):
        Connection(Input(n=4, traces=True), LIFNodes(n=3, traces=True), w=torch.rand(4, 3), wmin=0.0, wmax=wmax,
                   update_rule=WeightDependentPostPre, nu=(0.1, 0.1))


def test_refusals_that_stay():
    from bindsnet_amd.learning import PostPre, Rmax
    from bindsnet_amd.learning.MCC_learning import PostPre as MccPostPre
    from bindsnet_amd.network.nodes import Input, LIFNodes, SRM0Nodes
    from bindsnet_amd.network.topology import Connection, Conv2dConnection, MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Weight
    nu = [torch.full((3,), 0.1), torch.full((3,), 0.1)]
    with pytest.raises(NotImplementedError, match="per-synapse tensor learning rates are not supported"):
        Connection(Input(n=4, traces=True, traces_additive=True), SRM0Nodes(n=3), update_rule=Rmax, nu=nu)
    with pytest.raises(NotImplementedError, match="per-synapse tensor learning rates are not supported"):
        Conv2dConnection(Input(shape=[1, 6, 6], traces=True), LIFNodes(shape=[2, 4, 4], traces=True), kernel_size=3, update_rule=PostPre,
                         nu=[torch.full((2, 1, 3, 3), 0.1)] * 2)
    with pytest.raises(NotImplementedError, match="tensor norms are not supported on a torch.float16 Weight"):
        Weight("weight", torch.rand(4, 3).half(), value_dtype=torch.float16, norm=torch.ones(3))
    X, Y = Input(n=4, traces=True), LIFNodes(n=3, traces=True)
    feat = Weight("weight", torch.rand(4, 3).half() * 0.5, value_dtype=torch.float16, range=[torch.zeros(4, 3), torch.ones(4, 3)],
                  nu=[0.1, 0.1], learning_rule=MccPostPre)
    conn = MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat])
    with pytest.raises(NotImplementedError, match="per-synapse clamp ranges are not supported"):
        conn.pipeline[0].learning_rule._bounds(tensors=True)


def test_multi_device_modes_refuse_tensor_constants():
    from bindsnet_amd import parallel
    n = ns()
    for case, message in (("dense_postpre", "per-synapse tensor learning rates"), ("mcc_postpre", "per-synapse clamp ranges")):
        net = SC.build_run(n, case)
        for fn in (lambda: parallel.column_shard(net, 0, 2), lambda: parallel.sharded_run(net, {"X": torch.zeros(2, 3, SC.R_S, dtype=torch.uint8)}, 2)):
            with pytest.raises(NotImplementedError, match=message):
                fn()
    net = SC.build_run(n, "mcc_postpre")
    rule = net.connections[("X", "Y")].pipeline[0].learning_rule
    rule.min, rule.max = 0.0, 4.0
    with pytest.raises(NotImplementedError, match="tensor norms are not supported"):
        parallel._refuse(net, "sharded_run")


def test_drawn_weights_follow_tensor_bounds():
    """Connection(wmin=tensor, wmax=tensor) without `w=` (topology.py:309-318): wmin + rand * (wmax - wmin); clamped when a bound is infinite."""
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Connection
    lo, hi = torch.rand(5, 4) * 0.2, 0.5 + torch.rand(5, 4) * 0.2
    torch.manual_seed(3)
    conn = Connection(Input(n=5), LIFNodes(n=4), wmin=lo, wmax=hi)
    torch.manual_seed(3)
    assert torch.equal(conn.w.data, lo + torch.rand(5, 4) * (hi - lo))
    hi2 = hi.clone()
    hi2[0, 0] = float("inf")
    torch.manual_seed(3)
    conn = Connection(Input(n=5), LIFNodes(n=4), wmin=lo, wmax=hi2)
    torch.manual_seed(3)
    assert torch.equal(conn.w.data, torch.clamp(torch.rand(5, 4), lo, hi2))


def test_edits_and_copies_carry_the_constants(tmp_path):
    from bindsnet_amd.network import load
    n = ns()
    net = SC.build_run(n, "dense_postpre")
    ref = SC.run_run(n, SC.build_run(n, "dense_postpre"), "dense_postpre", n_in=1)
    path = str(tmp_path / "net.pt")
    net.save(path)
    for copy in (load(path), net.clone()):
        conn = copy.connections[("X", "Y")]
        assert conn.wmin.shape == (SC.R_S, SC.R_N) and conn.update_rule.nu.shape == (2, SC.R_N) and conn.norm.shape == (SC.R_N,)
        got = SC.run_run(n, copy, "dense_postpre", n_in=1)
        assert np.array_equal(got[0]["raster"], ref[0]["raster"]) and np.array_equal(bits(got[0]["w"]), bits(ref[0]["w"]))
    # an in-place edit of a bound, and its replacement, are seen by the next run
    for edit in (lambda c: c.wmax.fill_(0.3), lambda c: setattr(c, "wmax", torch.nn.Parameter(torch.full((SC.R_S, SC.R_N), 0.3), requires_grad=False))):
        net = SC.build_run(n, "dense_postpre")
        conn = net.connections[("X", "Y")]
        conn.norm = None
        SC.run_run(n, net, "dense_postpre", n_in=1)
        assert float(conn.w.max()) > 0.3
        edit(conn)
        SC.run_run(n, net, "dense_postpre", n_in=1)
        assert float(conn.w.max()) <= float(np.float32(0.3))
