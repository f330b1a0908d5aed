"""SRM0Nodes and Rmax on the MI355X (csrc/snn_srm0.hip).

The device's expf and torch's exp are two different 1-ulp functions, so `rho` and `s_prob` agree to a few ulp and not to the bit;
everything discrete must still agree exactly.  The criteria:

  * bit for bit: rasters, per-step v, refrac_count, traces and the generator state after the run.  In the Rmax cases v gets 2e-5
    absolute: the current is a sum of at most 40 addends of magnitude at most 1 whose order the host's BLAS does not document, and 40
    roundings of partial sums of at most 8 give at most 1.9e-5;
  * s_prob within DELTA_P = 8 * 2^-24 absolute in the direct, grid and mcc cases: the inputs of the first exp are identical, two 1-ulp
    functions differ by at most 2 ulp in rho, and through d/drho (1 - e^-rho) <= 1 and rho e^-rho <= 0.37 that stays under 3e-7.  In the
    Rmax cases DELTA_P_RULE = 2^-19: the v slack adds 0.37 * 2e-5 / d_thresh.  The draw margins the fixtures were generated with
    (srm0_cases.MARGIN) are 2^-20 = 2 * DELTA_P and 2^-14 = 32 * DELTA_P_RULE (the least margin a direct fixture actually holds is
    1.43e-6, three times DELTA_P), so a difference inside the bounds cannot flip a spike and the rasters may be required exactly;
  * Rmax state: |d e| <= tol_e = delta_p * max(x_src) * tc_e_trace / dt (the term's derivative in s_prob is at most 1, the trace's
    geometric memory is tc_e_trace / dt steps) and |d w| <= T * nu0 * |reward| * tol_e, computed from the case's own parameters and
    recorded source trace; the weights must have moved by more than 100 * tol_w somewhere.

Every fixture case runs on the generic plan, whole, in two halves, and one step per run() (which exposes every step's s_prob).  Against
the host path (pinned to the same fixtures by tests/test_srm0_host.py): standalone forward(), clamp / unclamp / injects_v, Rmax at two
more weight shapes."""
import numpy as np
import pytest
import torch

import srm0_cases as SC
from test_srm0_host import _bits, build, check_snapshots, gold, same

pytestmark = pytest.mark.gpu
DEV = "cuda"
DELTA_P, DELTA_P_RULE, V_RULE = 8 * 2.0 ** -24, 2.0 ** -19, 2e-5


@pytest.fixture(autouse=True)
def few_host_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(4, n))
    yield
    torch.set_num_threads(n)


def tolerances(name, r):
    """The device criteria of input `r` of a case (module docstring)."""
    c = SC.CASES[name]
    if not c.get("rule"):
        return dict(p=DELTA_P)
    g = gold(name)
    x_max = max(float(g[f"r{k}_rx"].max()) for k in range(r + 1))
    tol_e = DELTA_P_RULE * x_max * 25.0 / c.get("dt", 1.0)
    tol_w = (r + 1) * c["T"] * SC.NU * abs(c["reward"]) * tol_e
    return dict(p=DELTA_P_RULE, v=V_RULE, e=tol_e, w=tol_w)


def run_and_check(name, mode):
    from bindsnet_amd.network.monitors import Monitor
    net = build(name).to(DEV)
    snaps = SC.run_case(net, name, Monitor, device=DEV, mode=mode)
    assert net.last_plan == "generic"
    c, g = SC.CASES[name], gold(name)
    for r, s in enumerate(snaps):
        tol = tolerances(name, r)
        for L in SC.srm0_layers(name):
            spikes = s[L + "_raster"]
            assert 0 < spikes.sum() < spikes.size, "vacuous"
            for key in ("prec", "sprob"):
                if f"{L}_{key}" in s:
                    d = np.abs(s[f"{L}_{key}"].astype(np.float64) - g[f"r{r}_{L}_{key}"].astype(np.float64)).max()
                    print(f"case {name} input {r} {L} {key}: largest |s_prob - reference| = {d:.3g} (bound {tol['p']:.3g})")
        if c.get("rule"):
            print(f"case {name} input {r}: largest |e - reference| = {np.abs(s['e'] - g[f'r{r}_e']).max():.3g} (bound {tol['e']:.3g}), "
                  f"|w - reference| = {np.abs(s['w'] - g[f'r{r}_w']).max():.3g} (bound {tol['w']:.3g}), "
                  f"|v - reference| = {np.abs(s['Y_vrec'] - g[f'r{r}_Y_vrec']).max():.3g} (bound {tol['v']:.3g})")
            assert np.abs(g[f"r{r}_w"] - g["w0"]).max() > 100 * tol["w"], "the weights did not move far enough for the bound to mean anything"
        check_snapshots(name, [s], first=r, tol=tol)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_device_reproduces_reference_fixture(name):
    run_and_check(name, "whole")


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_every_step_s_prob_on_the_device(name):
    """One step per run(): every step's s_prob against the fixture's, and T generator hand-overs instead of one."""
    run_and_check(name, "steps")


@pytest.mark.parametrize("name", ["d_b2n313_w5", "d_b5n257_w623", "pervec", "dt05", "two", "mcc", "rmax_decay", "rmax_local"])
def test_two_half_runs_equal_one_whole_run(name):
    run_and_check(name, "halves")


# ------------------------------------------------------------------ against the host path
def _layer(n, B, dev, **kw):
    from bindsnet_amd.network.nodes import SRM0Nodes
    layer = SRM0Nodes(n=n, traces=True, **kw)
    layer.compute_decays(1.0)
    layer.set_batch_size(B)
    layer.to(dev)
    layer.set_batch_size(B)
    return layer


@pytest.mark.parametrize("B,n,T", [(3, 70, 20), (1, 255, 20), (5, 257, 20), (33, 1024, 6)])
def test_standalone_forward_equals_the_host_step(B, n, T):
    """(33, 1024): 33 792 draws, more than fifty twists per step."""
    cur = (-0.5 + 3.5 * np.random.default_rng(B * n).random((T, B, n), dtype=np.float32)).astype(np.float32)
    kw = dict(lbound=-70.25, refrac=3, thresh=torch.from_numpy((-50.0 + np.random.default_rng(n).standard_normal(n)).astype(np.float32))) \
        if n == 257 else dict(refrac=2)
    rec = {}
    for dev in ("cpu", DEV):
        torch.manual_seed(1000 + n)
        torch.rand(B)
        layer = _layer(n, B, dev, **kw)
        ss, pp = [], []
        for t in range(T):
            layer.forward(torch.from_numpy(cur[t].copy()).to(dev))
            ss.append(layer.s.cpu().numpy().astype(np.uint8).copy())
            pp.append(layer.s_prob.cpu().numpy().copy())
        rec[dev] = (np.stack(ss), np.stack(pp), layer, torch.get_rng_state())
    (s0, p0, l0, g0), (s1, p1, l1, g1) = rec["cpu"], rec[DEV]
    assert 0 < s0.sum() < s0.size, "vacuous"
    bad = np.flatnonzero((s0 != s1).reshape(T, -1).any(1))
    assert bad.size == 0, f"B={B} n={n}: spikes differ first at step {bad[:1]}"
    d = np.abs(p0.astype(np.float64) - p1).max()
    print(f"B={B} n={n}: largest |s_prob - host| = {d:.3g} (bound {DELTA_P:.3g})")
    assert d <= DELTA_P
    for k in ("v", "refrac_count", "x"):
        same(getattr(l1, k).cpu().numpy(), getattr(l0, k).numpy(), f"B={B} n={n}: {k}")
    # rho = rho_0 * exp(a) from identical a (v is exact): two 1-ulp exponentials are at most 2 ulp apart, the multiply keeps that
    # within 4 * 2^-23 relative.  It is the value BEFORE the reset, so it is not what the final v would give where a neuron spiked.
    r0, r1 = l0.rho.numpy().astype(np.float64), l1.rho.cpu().numpy().astype(np.float64)
    assert tuple(l1.rho.shape) == (B, n) and (np.abs(r1 - r0) <= 4 * 2.0 ** -23 * r0).all(), "rho differs from the host path's"
    assert not np.allclose(r0, l0.s_prob.numpy()), "rho and s_prob are different quantities"
    assert torch.equal(g0, g1), "the generator stands elsewhere than after the host steps"


def test_clamp_unclamp_injects_v_equal_the_host_path():
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.monitors import Monitor
    from bindsnet_amd.network.nodes import SRM0Nodes
    T, B, n = 20, 3, 45
    rng = np.random.default_rng(9)
    cur = (-0.5 + 3.0 * rng.random((T, B, n), dtype=np.float32)).astype(np.float32)
    clamp = torch.from_numpy(rng.random((T, n)) < 0.05)
    unclamp = torch.from_numpy(rng.random(n) < 0.2)
    inject = torch.from_numpy((rng.random((T, n), dtype=np.float32) - np.float32(0.3)).astype(np.float32))
    out = {}
    for dev in ("cpu", DEV):
        torch.manual_seed(77)
        net = Network(batch_size=B)
        net.add_layer(SRM0Nodes(n=n, traces=True, lbound=-70.5), "Y")
        mon = Monitor(net.layers["Y"], ["s", "v"], time=T)
        net.add_monitor(mon, "m")
        net.to(dev)
        net.run({"Y": torch.from_numpy(cur.copy()).to(dev)}, time=T, clamp={"Y": clamp}, unclamp={"Y": unclamp}, injects_v={"Y": inject})
        Y = net.layers["Y"]
        out[dev] = (mon.get("s").cpu().numpy().astype(np.uint8), mon.get("v").cpu().numpy(), Y.v.cpu().numpy(), Y.refrac_count.cpu().numpy(),
                    Y.x.cpu().numpy(), Y.s_prob.cpu().numpy(), torch.get_rng_state())
    assert net.last_plan == "generic"
    a, b = out["cpu"], out[DEV]
    assert 0 < a[0].sum() < a[0].size, "vacuous"
    assert np.array_equal(a[0], b[0]), "monitored spikes differ"
    for k, what in ((1, "per-step v"), (2, "v"), (3, "refrac_count"), (4, "trace")):
        same(b[k], a[k], what)
    assert np.abs(a[5].astype(np.float64) - b[5]).max() <= DELTA_P
    assert torch.equal(a[6], b[6])
    with pytest.raises(NotImplementedError, match="monitoring"):
        net.add_monitor(Monitor(net.layers["Y"], ["s_prob"], time=T), "p")
        net.run({"Y": torch.from_numpy(cur.copy()).to(DEV)}, time=T)


def _rmax_graph(S, n, seed):
    from bindsnet_amd.learning import Rmax
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, SRM0Nodes
    from bindsnet_amd.network.topology import Connection
    rng = np.random.default_rng(seed)
    net = Network()
    X, Y = Input(n=S, traces=True, traces_additive=True), SRM0Nodes(n=n, traces=True)
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    w = (rng.random((S, n), dtype=np.float32) * np.float32(8.0 / S)).astype(np.float32)
    net.add_connection(Connection(X, Y, w=torch.from_numpy(w), update_rule=Rmax, nu=1e-3, weight_decay=1e-3, wmin=-8.0 / S, wmax=8.0 / S), "X", "Y")
    return net


RMAX_T, RMAX_SEED = 25, {70: 5, 257: 5}
RMAX_MARGIN = 16 * DELTA_P_RULE          # what every host draw keeps from its s_prob: the factor the fixtures' Rmax margin has over DELTA_P_RULE


def _rmax_run(dev, S, n, seed, x):
    """T runs of one step each; on the host every step's draws are replayed and their least distance to s_prob is returned."""
    torch.manual_seed(seed)
    net = _rmax_graph(S, n, seed).to(dev)
    Y, rule = net.layers["Y"], net.connections[("X", "Y")].update_rule
    ss, pp, xs, margin = [], [], [], np.inf
    for t in range(x.shape[0]):
        before = torch.get_rng_state()
        net.run({"X": torch.from_numpy(x[t:t + 1].copy()).to(dev)}, time=1, reward=0.75)
        if dev == "cpu":
            after = torch.get_rng_state()
            torch.set_rng_state(before)
            margin = min(margin, float((torch.rand_like(Y.s_prob) - Y.s_prob).abs().min()))
            assert torch.equal(torch.get_rng_state(), after)
        ss.append(Y.s.cpu().numpy().astype(np.uint8).copy())
        pp.append(Y.s_prob.cpu().numpy().copy())
        xs.append(float(net.layers["X"].x.max()))
    return (np.stack(ss), np.stack(pp), Y.v.cpu().numpy(), rule.eligibility_trace.cpu().numpy(), net.connections[("X", "Y")].w.detach().cpu().numpy(),
            torch.get_rng_state(), margin, max(xs), net.last_plan)


@pytest.mark.parametrize("S,n", [(70, 33), (257, 65)])
def test_rmax_at_other_weight_shapes_equals_the_host_path(S, n):
    """The fixture cases' device criteria (module docstring) at two more weight shapes, the host path standing in for the reference:
    v within V_RULE = 2e-5, s_prob within DELTA_P_RULE = 2^-19, e and w within the bounds derived from it, everything discrete exact.
    The argument for V_RULE carries over: |w| <= 8 / S (the connection's bounds) and at most A active sources in a step make a current a
    sum of at most A addends with partial sums below 8 A / S < 4, so two summation orders differ by at most A roundings of ulp(2..4) = 2^-22:
    A * 2^-22, which the test checks to be under V_RULE for its input.  One step per run() on both sides, so that every step's host draws
    can be replayed: each keeps 16 * DELTA_P_RULE from its s_prob (a property of the seed, asserted first), the fixtures' own factor."""
    T, seed = RMAX_T, RMAX_SEED[S]
    x = (np.random.default_rng(seed + 100).random((T, 1, S)) < 0.25).astype(np.uint8)
    A = int(x.sum(axis=2).max())
    assert 8.0 * A / S < 4.0 and A * 2.0 ** -22 <= V_RULE, (A, S)
    a, b = _rmax_run("cpu", S, n, seed, x), _rmax_run(DEV, S, n, seed, x)
    assert b[8] == "generic" and a[6] >= RMAX_MARGIN, f"the host draws come within {a[6]:.3g} of s_prob (needed {RMAX_MARGIN:.3g}): choose another seed"
    assert 0 < a[0].sum() < a[0].size, "vacuous"
    assert np.array_equal(a[0], b[0]), "spikes differ"
    tol_e = DELTA_P_RULE * a[7] * 25.0
    tol_w = T * 1e-3 * 0.75 * tol_e
    figs = [np.abs(a[k].astype(np.float64) - b[k]).max() for k in (1, 2, 3, 4)]
    print(f"S={S} n={n}: |s_prob| {figs[0]:.3g} (bound {DELTA_P_RULE:.3g}), |v| {figs[1]:.3g} ({V_RULE:.3g}), |e| {figs[2]:.3g} ({tol_e:.3g}), "
          f"|w| {figs[3]:.3g} ({tol_w:.3g})")
    assert figs[0] <= DELTA_P_RULE and figs[1] <= V_RULE and figs[2] <= tol_e and figs[3] <= tol_w
    w0 = _rmax_graph(S, n, seed).connections[("X", "Y")].w.numpy()
    assert np.abs(a[4] - w0).max() > 100 * tol_w, "the weights did not move far enough for the bound to mean anything"
    assert torch.equal(a[5], b[5]), "the generator stands elsewhere than after the host run"


def test_standalone_rmax_update_equals_the_host_path():
    """Rmax.update() on its own (ops.rmax_step), hand-stepped beside the layers' forward(): the SRM0 layer is driven by a given current,
    so v is exact and s_prob within DELTA_P; e and w within the bounds that follow from DELTA_P."""
    from bindsnet_amd.learning import Rmax
    from bindsnet_amd.network.nodes import Input, SRM0Nodes
    from bindsnet_amd.network.topology import Connection
    S, n, T, reward = 37, 70, 20, -0.5
    rng = np.random.default_rng(12)
    xs = (rng.random((T, 1, S)) < 0.3).astype(np.uint8)
    cur = (-0.5 + 3.5 * rng.random((T, 1, n), dtype=np.float32)).astype(np.float32)
    w0 = (rng.random((S, n), dtype=np.float32) * np.float32(0.2)).astype(np.float32)
    rec = {}
    for dev in ("cpu", DEV):
        torch.manual_seed(31)
        X, Y = Input(n=S, traces=True, traces_additive=True), SRM0Nodes(n=n, traces=True)
        conn = Connection(X, Y, w=torch.from_numpy(w0.copy()), update_rule=Rmax, nu=1e-3, weight_decay=1e-3, wmin=0.0, wmax=0.18)
        conn.dt = 1.0
        for l in (X, Y):
            l.compute_decays(1.0)
            l.set_batch_size(1)
            l.to(dev)
            l.set_batch_size(1)
        conn.to(dev)
        ss = []
        for t in range(T):
            X.forward(torch.from_numpy(xs[t].copy()).to(dev))
            Y.forward(torch.from_numpy(cur[t].copy()).to(dev))
            conn.update(reward=reward)
            ss.append(Y.s.cpu().numpy().astype(np.uint8).copy())
        rec[dev] = (np.stack(ss), Y.v.cpu().numpy(), conn.update_rule.eligibility_trace.cpu().numpy(), conn.w.detach().cpu().numpy(),
                    float(X.x.max()), torch.get_rng_state())
    a, b = rec["cpu"], rec[DEV]
    assert 0 < a[0].sum() < a[0].size, "vacuous"
    assert np.array_equal(a[0], b[0]), "spikes differ"
    same(b[1], a[1], "v")
    tol_e = DELTA_P * a[4] * 25.0                     # delta_p * max(x_src) * tc_e_trace / dt (module docstring)
    tol_w = T * 1e-3 * abs(reward) * tol_e
    de, dw = np.abs(a[2].astype(np.float64) - b[2]).max(), np.abs(a[3].astype(np.float64) - b[3]).max()
    print(f"standalone Rmax: |e| {de:.3g} (bound {tol_e:.3g}), |w| {dw:.3g} (bound {tol_w:.3g})")
    assert de <= tol_e and dw <= tol_w
    assert np.abs(a[3] - w0).max() > 100 * tol_w and (a[3] == 0.0).any() and (a[3] == np.float32(0.18)).any(), "not moved, or not clamped at both bounds"
    assert torch.equal(a[5], b[5])


def test_rmax_at_batch_two_and_tensor_eps_0_raise_on_the_device():
    from bindsnet_amd.learning import Rmax
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, SRM0Nodes
    from bindsnet_amd.network.topology import Connection
    net = Network(batch_size=2)
    X, Y = Input(n=8, traces=True, traces_additive=True), SRM0Nodes(n=4, traces=True)
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(Connection(X, Y, w=torch.rand(8, 4), update_rule=Rmax, nu=1e-3), "X", "Y")
    net.to(DEV)
    v0, st = net.layers["Y"].v.clone(), torch.get_rng_state()
    with pytest.raises(NotImplementedError, match=r"view\(-1\)"):
        net.run({"X": torch.ones(3, 2, 8, dtype=torch.uint8, device=DEV)}, time=3, reward=1.0)
    assert torch.equal(net.layers["Y"].v, v0) and torch.equal(torch.get_rng_state(), st)
    net = Network()
    net.add_layer(SRM0Nodes(n=4, eps_0=torch.full((4,), 1.5)), "Y")
    net.to(DEV)
    with pytest.raises(NotImplementedError, match="eps_0"):
        net.run({"Y": torch.ones(2, 1, 4, device=DEV)}, time=2)
    assert torch.equal(torch.get_rng_state(), st)
