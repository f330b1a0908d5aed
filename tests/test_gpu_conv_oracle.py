"""Every device plan of Input -> Conv2dConnection [PostPre] -> LIFNodes against the stepped CPU oracle (tests/conv_oracle_run.py, itself pinned to
the reference by tests/test_conv_oracle_run.py), bit for bit, over two consecutive runs: the spike raster, v, refrac_count, s, both traces and the
weights.  test_gpu_convpp.py checks fused == generic at shapes where a workgroup's filter elements fit its threads; the shapes here are chosen
around the fused kernel's limits instead -- filter elements per workgroup (nel = channels per workgroup * Cin*KH*KW) above, at and below its
thread count NT, NT not a multiple of 256, output rows of 32 pixels, 1024 pixels, one output pixel, 33 samples -- and the plans are checked
against the oracle, not against each other, so one that is wrong in the same way as another cannot pass.

Each variant asserts the plan it took: a forced chunk size that quietly fell back to the generic plan would prove nothing about the fused kernel."""
import numpy as np
import pytest
import torch

import synth
from conv_oracle_run import ConvOracleRun
from dt_cases import again, run_time

pytestmark = pytest.mark.gpu
DEV = "cuda"
u8 = np.uint8
FUSED, GENERIC, CONVLIF = "convpp-fused", "generic", "convlif-fused"


def case(B, T, Cin, H, W, Cout, k, stride, pad, dens, w, plans, vmax=1, nu=(1e-4, 5e-4), wmin=None, wmax=None, wd=0.0, learning=True,
         vmon=False, dt=1.0, refrac=None):
    """plans: the plan of (auto, 2, 4, 8 channels per workgroup), worked out from convpp_match / convpp_threads / convpp_lds.
    dt: the network's timestep (T steps are `time = T * dt`); refrac: the LIF layer's refractory period (None: the class default)."""
    return dict(B=B, T=T, Cin=Cin, H=H, W=W, Cout=Cout, k=k if isinstance(k, tuple) else (k, k), stride=stride, pad=pad, dens=dens,
                w=w, plans=plans, vmax=vmax, nu=nu, wmin=wmin, wmax=wmax, wd=wd, learning=learning, vmon=vmon, dt=dt, refrac=refrac)


ALL_FUSED = (FUSED, FUSED, FUSED, FUSED)
#   nel at 2 / 4 / 8 channels per workgroup, and NT (threads = max(256, OH*OW rounded up to 64)):
CASES = {
    # conv_mnist.py's defaults without the norm: 4x4 outputs, stride 4 (no event lists); 512 / 1024 / 2048 vs 256
    "k16_s4": case(8, 14, 1, 28, 28, 25, 16, 4, 0, 0.08, (-0.05, 0.18), ALL_FUSED, vmon=True),
    # the event-list path; 512 / 1024 / 1536 vs 256, the last chunk partial at 4 and 8, OW = 13
    "k16_s1": case(4, 14, 1, 28, 28, 6, 16, 1, 0, 0.08, (-0.05, 0.18), ALL_FUSED),
    # spike values 1..3: the dense-byte partial sums (conv_pp_dense)
    "k16_s1_bytes": case(4, 14, 1, 28, 28, 6, 16, 1, 0, 0.06, (-0.05, 0.2), ALL_FUSED, vmax=3, vmon=True),
    # three input channels, general window form; 294 / 588 / 735 vs 256, E % 32 == 31 (the batch reduction's tail elements)
    "rgb_k7_s2_p1": case(4, 14, 3, 28, 28, 5, 7, 2, 1, 0.12, (-0.05, 0.4), ALL_FUSED),
    # 72 / 144 / 288 vs 256: only 8 channels per workgroup exceeds NT
    "k6": case(3, 16, 1, 16, 16, 8, 6, 1, 0, 0.15, (-0.05, 0.6), ALL_FUSED),
    # 128 / 256 / 512 vs 256: nel == NT exactly at 4
    "k8_exact": case(3, 16, 1, 16, 16, 8, 8, 1, 0, 0.12, (-0.05, 0.5), ALL_FUSED),
    # non-square kernel; 66 / 132 / 264 vs 256 (NT + 8 at 8)
    "nonsquare_3x11": case(3, 16, 1, 20, 24, 8, (3, 11), 1, 0, 0.2, (-0.05, 0.8), ALL_FUSED),
    # 17x17 outputs: NT = 320; 512 / 1024 / 1024; full 32-bit input row words
    "k16_32x32": case(2, 14, 1, 32, 32, 4, 16, 1, 0, 0.08, (-0.05, 0.18), ALL_FUSED),
    # 32x32 outputs: window masks at bit 31, NT = 1024 (the pixel limit), padding on both sides; 18 / 36 / 54
    "full_rows_1024": case(2, 16, 1, 32, 32, 6, 3, 1, 1, 0.3, (-0.1, 2.0), ALL_FUSED, vmon=True),
    # one output pixel, 33 samples (two cascade blocks and a remainder); 288 vs 256 at 2, 4 and 8 exceed 150 KB of LDS
    "whole_image_kernel_b33": case(33, 12, 1, 12, 12, 3, 12, 1, 0, 0.1, (-0.05, 0.5), (FUSED, FUSED, GENERIC, GENERIC)),
    # 16 input channels: the image (3136 words) exceeds 4 * NT, only the generic plan takes it (k_conv2d with 50 KB of filters)
    "cin16_28x28": case(2, 12, 16, 28, 28, 32, 5, 1, 0, 0.05, (-0.05, 0.25), (GENERIC,) * 4),
    # the variants of the rule on wide cases: no learning (the fused kernel with learning off), clamps with weight decay, one term only
    "k16_s1_learning_off": case(4, 14, 1, 28, 28, 6, 16, 1, 0, 0.08, (-0.05, 0.18), ALL_FUSED, learning=False),
    "k16_s4_clamp_decay": case(8, 14, 1, 28, 28, 25, 16, 4, 0, 0.08, (-0.05, 0.18), ALL_FUSED, nu=(2e-4, 1e-3), wmin=0.0, wmax=0.2,
                               wd=0.01),
    "rgb_k7_clamp_decay": case(4, 14, 3, 28, 28, 5, 7, 2, 1, 0.12, (-0.05, 0.4), ALL_FUSED, nu=(2e-4, 3e-4), wmin=0.0, wmax=0.3,
                               wd=0.005),
    "k16_32x32_only_pre": case(2, 14, 1, 32, 32, 4, 16, 1, 0, 0.08, (-0.05, 0.18), ALL_FUSED, nu=(3e-4, 0.0)),
    "k16_32x32_only_post": case(2, 14, 1, 32, 32, 4, 16, 1, 0, 0.08, (-0.05, 0.18), ALL_FUSED, nu=(0.0, 1e-3)),
    # dt != 1: both whole-run kernels keep the refractory counter in registers and step it by dt; the decays of v and of both traces
    # are exp(-dt / tc).  k16_s1 over 50 steps: ten steps of refractory period at dt 0.5; at dt 2.0 with refrac 5 the counter runs 5, 3, 1, -1
    "k16_s1_dt05": case(4, 50, 1, 28, 28, 6, 16, 1, 0, 0.08, (-0.05, 0.18), ALL_FUSED, vmon=True, dt=0.5),
    "k16_s1_dt2_refrac5": case(4, 50, 1, 28, 28, 6, 16, 1, 0, 0.08, (-0.05, 0.18), ALL_FUSED, vmon=True, dt=2.0, refrac=5),
}
VARIANTS = {"auto": 0, "cc2": 1, "cc4": 2, "cc8": 3, "generic": None}
CONVLIF_CASES = ["k16_s1", "rgb_k7_s2_p1", "k16_32x32", "full_rows_1024", "k16_s1_dt05", "k16_s1_dt2_refrac5"]


def geometry(c):
    (KH, KW), s, p = c["k"], c["stride"], c["pad"]
    return (c["H"] + 2 * p - KH) // s + 1, (c["W"] + 2 * p - KW) // s + 1


def w0(c):
    return synth.uniform_f32(7, (c["Cout"], c["Cin"]) + c["k"], *c["w"])


def inputs(c, r):
    sp = synth.dense_spikes(60 + r, (c["T"], c["B"], c["Cin"], c["H"], c["W"]), c["dens"])
    if c["vmax"] > 1:
        sp = (sp * np.random.RandomState(3 + r).randint(1, c["vmax"] + 1, size=sp.shape)).astype(u8)
    return sp


def build(c, rule=True):
    from bindsnet_amd.learning import PostPre
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Conv2dConnection
    OH, OW = geometry(c)
    net = Network(dt=c["dt"], batch_size=c["B"], learning=c["learning"])
    net.add_layer(Input(shape=(c["Cin"], c["H"], c["W"]), traces=True), "X")
    net.add_layer(LIFNodes(shape=(c["Cout"], OH, OW), traces=True, **({} if c["refrac"] is None else {"refrac": c["refrac"]})), "Y")
    kw = dict(kernel_size=c["k"], stride=c["stride"], padding=c["pad"], w=torch.from_numpy(w0(c)))
    if rule:
        kw.update(update_rule=PostPre, nu=c["nu"], weight_decay=c["wd"])
        if c["wmin"] is not None:
            kw["wmin"] = c["wmin"]
        if c["wmax"] is not None:
            kw["wmax"] = c["wmax"]
    net.add_connection(Conv2dConnection(net.layers["X"], net.layers["Y"], **kw), "X", "Y")
    return net


_ORACLE = {}


def oracle_runs(name, rule=True, n_runs=2):
    key = (name, rule)
    if key not in _ORACLE:
        c = CASES[name]
        orc = ConvOracleRun(build(c, rule), c["B"])
        _ORACLE[key] = [orc.run(inputs(c, r), learning=c["learning"], voltages=c["vmon"]) for r in range(n_runs)]
    return _ORACLE[key]


def device_runs(name, rule=True, n_runs=2):
    from bindsnet_amd.network.monitors import Monitor
    c = CASES[name]
    net = build(c, rule)
    T = c["T"]
    mons = {"s": Monitor(net.layers["Y"], ["s"], time=T)}
    if c["vmon"]:
        mons["v"] = Monitor(net.layers["Y"], ["v"], time=T)
    for n_, m in mons.items():
        net.add_monitor(m, n_)
    net.to(DEV)
    out, plans = [], []
    for r in range(n_runs):
        net.run({"X": torch.from_numpy(inputs(c, r)).to(DEV)}, time=run_time(T, c["dt"]))
        X, Y = net.layers["X"], net.layers["Y"]
        host = lambda t: t.detach().cpu().numpy().copy()
        st = dict(s=host(mons["s"].get("s")).astype(u8), v=host(Y.v), refrac_count=host(Y.refrac_count), sY=host(Y.s).astype(u8),
                  xY=host(Y.x), xX=host(X.x), W=host(net.connections[("X", "Y")].w))
        if c["vmon"]:
            st["vras"] = host(mons["v"].get("v"))
        out.append(st)
        plans.append(net.last_plan)
    return out, plans


def first_difference(got, want):
    """Index of the first element whose bits differ, or None."""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = g.view(u8).reshape(g.size, -1) != w.view(u8).reshape(w.size, -1)
    flat = np.flatnonzero(bad.any(axis=1))
    return None if flat.size == 0 else (np.unravel_index(flat[0], g.shape), flat.size)


def compare(got, want, W0, what):
    for k in sorted(want, key=lambda k: k != "W"):           # the weights first: a wrong update shows up in everything after it
        g = got[k].reshape(want[k].shape)
        d = first_difference(g, want[k])
        if d is None:
            continue
        idx, n = d
        if k == "W":
            co, taps = idx[0], W0.shape[1] * W0.shape[2] * W0.shape[3]
            tap = int(np.ravel_multi_index(idx[1:], W0.shape[1:]))
            frozen = int(np.count_nonzero((g == W0) & (want[k] != W0)))
            msg = (f"{what}: W differs first at (channel {co}, tap {tap} of {taps}): got {g[idx]!r}, oracle {want[k][idx]!r}; "
                   f"{n} elements differ, {frozen} of them still hold their initial value where the oracle's moved")
        else:
            msg = f"{what}: {k} differs first at {tuple(int(i) for i in idx)}: got {g[idx]!r}, oracle {want[k][idx]!r}; {n} elements differ"
        pytest.fail(msg)


def check_not_vacuous(name, runs, learning):
    c = CASES[name]
    assert sum(int(r["s"].sum()) for r in runs) > 0, f"{name}: no output spike in the oracle run"
    if c["dt"] != 1.0:
        # a refractory period ended and the neuron fired again, twice: neurons with three or more spikes in one sample of one run
        n = max(again(r["s"].reshape(c["T"], c["B"], -1)) for r in runs)
        assert n >= 10, f"{name}: only {n} neurons fire three times in the oracle run"
    if learning:
        # a frozen slice of filter elements could hide behind elements the oracle leaves alone: every channel's filter moves, in the first
        # and in the last half of its taps
        moved = (runs[-1]["W"] != w0(c)).reshape(c["Cout"], -1)
        half = moved.shape[1] // 2
        for co in range(c["Cout"]):
            assert moved[co, :half].any() and moved[co, half:].any(), f"{name}: channel {co}'s filter does not move in both halves"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(CASES))
def test_conv_postpre_plan_matches_stepped_oracle(name, variant, monkeypatch):
    from bindsnet_amd import _lib
    c = CASES[name]
    want = oracle_runs(name)
    check_not_vacuous(name, want, c["learning"])
    pi = VARIANTS[variant]
    expect = GENERIC if pi is None else c["plans"][pi]
    if variant.startswith("cc"):
        monkeypatch.setenv("SNN_CONVPP_CC", variant[2:])
    _lib.lib().snn_set_plan_mode(1 if pi is None else 0)
    try:
        got, plans = device_runs(name)
    finally:
        _lib.lib().snn_set_plan_mode(0)
    assert plans == [expect] * len(plans), f"{name} {variant}: plans {plans}, expected {expect}"
    W0 = w0(c)
    for r, (g, w) in enumerate(zip(got, want)):
        compare(g, w, W0, f"{name} {variant} ({expect}) run {r}")


@pytest.mark.parametrize("variant", ["auto", "generic"])
@pytest.mark.parametrize("name", CONVLIF_CASES)
def test_conv_without_rule_plan_matches_stepped_oracle(name, variant):
    """The same graph without an update rule: the whole-run plan convlif-fused, and the generic plan, against the oracle's no-learning run."""
    from bindsnet_amd import _lib
    want = oracle_runs(name, rule=False)
    check_not_vacuous(name, want, False)
    _lib.lib().snn_set_plan_mode(1 if variant == "generic" else 0)
    try:
        got, plans = device_runs(name, rule=False)
    finally:
        _lib.lib().snn_set_plan_mode(0)
    expect = GENERIC if variant == "generic" else CONVLIF
    assert plans == [expect] * len(plans), f"{name} {variant}: plans {plans}, expected {expect}"
    for r, (g, w) in enumerate(zip(got, want)):
        compare(g, w, w0(CASES[name]), f"{name} {variant} ({expect}, no rule) run {r}")
