"""The layer-major plan on the device (Network.layer_major, network/layer_major.py): snn_run_conv2d_sif_f32 -- a Conv2dConnection and its
SubtractiveResetIFNodes over the whole run in one launch -- and the time-chunked route with snn_sif_scan, against a plain float64
reference (weights on a 1/64 grid: every partial sum exact, so equality is exact) and, with randn weights, bit for bit against the
generic plan, after one run and after a second run without a reset.  The cases and what each is there for: tests/layer_major_cases.py."""
import numpy as np
import pytest
import torch

from layer_major_cases import CASES, build, byte2_frames, geometry, inputs_of, khw, options, reference, references, shapes, spike_input, weights

pytestmark = pytest.mark.gpu


def run_twice(net, xs):
    """Two runs without a reset; per run: every layer's train, then every layer's state."""
    from bindsnet_amd.network.monitors import Monitor
    out = []
    for x in xs:
        mons = {l: Monitor(layer, ["s"], time=x.shape[0]) for l, layer in net.layers.items() if l != "0"}
        for l, m in mons.items():
            net.add_monitor(m, "m" + l)
        net.run({"0": x.to("cuda")}, time=x.shape[0])
        trains = [mons[l].get("s").to(torch.uint8).cpu() for l in sorted(mons, key=int)]
        out.append((trains, state_of(net), net.last_plan))
        for l in mons:
            del net.monitors["m" + l]
    return out


def state_of(net):
    return [{k: getattr(net.layers[l], k).detach().float().cpu().clone() for k in ("s", "v", "refrac_count", "x", "summed")
             if isinstance(getattr(net.layers[l], k, None), torch.Tensor)} for l in sorted(net.layers, key=int) if l != "0"]


def takes_of(spec, T, B, k=0):
    from bindsnet_amd import ops
    cin, H, W = tuple(spec[0]) if k == 0 else shapes(spec)[k - 1]
    _, cout, kk, stride, pad = spec[1][k]
    return ops.run_conv2d_sif_takes(T, B, cin, H, W, cout, *khw(kk), stride, pad)


def assert_reaches_its_branch(name):
    """The case's geometry as tests/layer_major_cases.py restates it, and the restatement's `resident` against the library's own answer."""
    spec, T, B, opt, needs = CASES[name]
    if needs is not None:
        assert needs(geometry(spec)), geometry(spec)
    assert byte2_frames(name) == ([] if opt.get("analog") else [(r, min(f, T - 1)) for r, f in opt.get("two", ())])
    if not opt.get("analog"):
        assert takes_of(spec, T, B) == (0 if name == "refused_bytes" else 1 if geometry(spec)["resident"] else 2)


def assert_equals_the_reference(name, runs):
    """`runs` as run_twice gives them, of the case's network with its grid weights."""
    fired = 0
    for (want, state), (trains, st, plan) in zip(references(name)[2], runs):   # (the second run starts from a non-zero frame and state)
        assert plan == "layer-major"
        fired += sum(int(w.sum()) for w in want)
        for k, (got, w) in enumerate(zip(trains, want)):
            assert torch.equal(got.reshape(w.shape), w), f"train of layer {k + 1}"
            assert torch.equal(st[k]["v"].double().reshape(state["v"][k].shape), state["v"][k]), f"v of layer {k + 1}"
            assert torch.equal(st[k]["refrac_count"].double().reshape(state["rc"][k].shape), state["rc"][k]), f"refrac_count of layer {k + 1}"
            if CASES[name][3].get("traces"):
                assert torch.equal(st[k]["x"].double().reshape(state["x"][k].shape), state["x"][k]), f"x of layer {k + 1}"
        assert torch.equal(st[-1]["summed"].double().reshape(state["summed"].shape), state["summed"])
    assert fired > 0                                               # (at T = 1 the first run sees only the zero start frame)


def assert_same_bits(runs, runs0, plans=("layer-major", "generic")):
    for (trains, st, plan), (trains0, st0, plan0) in zip(runs, runs0):
        assert (plan, plan0) == plans
        for k in range(len(trains)):
            assert torch.equal(trains[k], trains0[k]), f"train of layer {k + 1}"
        for k in range(len(st)):
            assert st[k].keys() == st0[k].keys()
            for key in st[k]:
                assert np.array_equal(st[k][key].numpy().view(np.uint32), st0[k][key].numpy().view(np.uint32)), f"{key} of layer {k + 1}"


_generic = {}


def generic_runs(name):
    """The generic plan's two runs of the case with randn weights: once per case."""
    if name not in _generic:
        spec, T, B, opt, _ = CASES[name]
        _generic[name] = run_twice(build(spec, weights(spec, 6, grid=False), B, False, **options(opt)).to("cuda"), inputs_of(name))
        assert sum(int(t.sum()) for trains0, _, _ in _generic[name] for t in trains0) > 0
    return _generic[name]


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_float64_reference(name):
    spec, T, B, opt, _ = CASES[name]
    assert_reaches_its_branch(name)
    ws, xs, _ = references(name)
    assert_equals_the_reference(name, run_twice(build(spec, ws, B, True, **options(opt)).to("cuda"), xs))


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_generic_plan_bit_for_bit(name):
    spec, T, B, opt, _ = CASES[name]
    assert_reaches_its_branch(name)
    runs = run_twice(build(spec, weights(spec, 6, grid=False), B, True, **options(opt)).to("cuda"), inputs_of(name))
    assert_same_bits(runs, generic_runs(name))


# ---- the time chunks of route 2

def route2_widths(name):
    """n of every layer whose connection the one-launch kernel does not take."""
    spec, T, B, opt, _ = CASES[name]
    return [int(np.prod(sh)) for k, (op, sh) in enumerate(zip(spec[1], shapes(spec)))
            if not (op[0] == "conv" and not (k == 0 and opt.get("analog")) and takes_of(spec, T, B, k))]


def chunk_length(T, B, n):
    """Tc as network/layer_major.py computes it, from the module's (patched) constants."""
    from bindsnet_amd.network import layer_major as lm
    return max(1, min(T, lm.CURRENTS_BUDGET_BYTES // (4 * B * n), lm.MAX_OPERATOR_BATCH // B))


# (what is patched, its value from (B, the widest route-2 layer's n), the Tc that layer must then get)
CHUNKS = {
    "Tc1": ("CURRENTS_BUDGET_BYTES", lambda B, n: 4 * B * n * 1, 1),
    "Tc2": ("CURRENTS_BUDGET_BYTES", lambda B, n: 4 * B * n * 2, 2),
    "Tc3": ("CURRENTS_BUDGET_BYTES", lambda B, n: 4 * B * n * 3 + 4 * B * n - 1, 3),      # (one byte short of four frames)
    "Tc6": ("CURRENTS_BUDGET_BYTES", lambda B, n: 4 * B * n * 6, 6),
    "budget0": ("CURRENTS_BUDGET_BYTES", lambda B, n: 0, 1),                               # the max(1, ...) floor
    "batch_B": ("MAX_OPERATOR_BATCH", lambda B, n: B, 1),
    "batch_2B+1": ("MAX_OPERATOR_BATCH", lambda B, n: 2 * B + 1, 2),
}


@pytest.mark.parametrize("chunks", list(CHUNKS))
@pytest.mark.parametrize("name", ("stack_bytes", "stack_analog", "refused_bytes", "stack_bytes_sparse", "stack_analog_sparse"))
def test_time_chunks_change_nothing(name, chunks, monkeypatch):
    """T = 7 in chunks of Tc: the loop over chunks, the start frame as a call of its own (alone in its chunk at Tc = 1), train[t0:t1]
    and several snn_sif_scan calls per layer.  stack_analog's first convolution (a real-valued input) and refused_bytes' (spike bytes,
    a shape the kernel refuses) go through the chunks too.  In the second run of stack_bytes and stack_analog the reference fires all
    the time from the second layer on, so there only v and summed tell; the _sparse twins, whose every layer fires some of the time in
    both runs (tests/test_layer_major_cases.py), are there for the trains."""
    from bindsnet_amd.network import layer_major as lm
    spec, T, B, opt, _ = CASES[name]
    assert (T, B) == (7, 3)
    generic = generic_runs(name)                                   # (the unpatched generic plan, which reads neither constant)
    widths = route2_widths(name)
    assert len(widths) == (1 if name == "refused_bytes" else 4 if opt.get("analog") else 3)
    what, value, Tc = CHUNKS[chunks]
    monkeypatch.setattr(lm, what, value(B, max(widths)))
    assert chunk_length(T, B, max(widths)) == Tc < T and all(chunk_length(T, B, n) >= Tc for n in widths)
    ws, xs, _ = references(name)
    assert_equals_the_reference(name, run_twice(build(spec, ws, B, True, **options(opt)).to("cuda"), xs))
    assert_same_bits(run_twice(build(spec, weights(spec, 6, grid=False), B, True, **options(opt)).to("cuda"), inputs_of(name)), generic)


# ---- how a run is fed and watched

PLUMB = (((3, 9, 9), [("conv", 20, 3, 1, 1), ("pool",), ("fc", 5)]), 3)      # (spec, B): routes 1, 2, 2
PLUMB_NUM = [(-4, 12), (-4, 12), (-8, 8)]                                     # (the fc reads some hundred spikes a step: a zero-mean range)


def plumbed(ws, lm, xs, times, watch=(), cast=None):
    """Runs of `times` steps on one network without a reset, spike monitors on the layers in `watch` (kept over all runs, time = the
    run's): per run ({layer: what its monitor holds}, state, plan)."""
    from bindsnet_amd.network.monitors import Monitor
    spec, B = PLUMB
    net = build(spec, ws, B, lm).to("cuda")
    out = []
    for x, T in zip(xs, times):
        for l in watch:
            net.add_monitor(Monitor(net.layers[l], ["s"], time=T), "m" + l)
        x = x.to("cuda")
        net.run({"0": x if cast is None else x.to(cast)}, time=T)
        out.append(({l: net.monitors["m" + l].get("s").to(torch.uint8).cpu() for l in watch}, state_of(net), net.last_plan))
    return out


@pytest.mark.parametrize("how", ("last_only", "unwatched", "input_watched", "longer_input", "bool_input", "T_7_3_7", "T_7_3_7_last_only",
                                 "T_7_3_7_unwatched"))
def test_how_a_run_is_fed_and_watched(how):
    """A monitor on the last layer only (the trains between live in the plan's scratch, and feed the next layer from there), none at
    all, one on the Input; an input longer than `time`; a bool input; runs of 7, 3 and 7 steps (the scratch is keyed by shape)."""
    spec, B = PLUMB
    times = (7, 3, 7) if how.startswith("T_7_3_7") else (7, 7)
    frames = [T + 3 if how == "longer_input" else T for T in times]
    xs = [spike_input(spec, F, B, 20 + i) for i, F in enumerate(frames)]
    watch = {"last_only": ("3",), "T_7_3_7_last_only": ("3",), "unwatched": (), "T_7_3_7_unwatched": (),
             "input_watched": ("0", "3")}.get(how, ("1", "2", "3"))
    cast = torch.bool if how == "bool_input" else None
    last = len(spec[1])

    ws = weights(spec, 5, grid=True, num=PLUMB_NUM)
    state = {}
    for x, T, (held, st, plan) in zip(xs, times, plumbed(ws, True, xs, times, watch, cast)):
        want = reference(spec, ws, x[:T], state)
        assert plan == "layer-major" and 0.05 <= float(want[-1].double().mean()) <= 0.95
        for l in watch:
            assert torch.equal(held[l].reshape(T, B, -1), (x[:T] if l == "0" else want[int(l) - 1]).reshape(T, B, -1)), f"train of layer {l}"
        for k in range(last):
            assert torch.equal(st[k]["v"].double().reshape(state["v"][k].shape), state["v"][k]), f"v of layer {k + 1}"
            assert torch.equal(st[k]["s"].double().reshape(state["s"][k + 1].shape), state["s"][k + 1]), f"s of layer {k + 1}"
        assert torch.equal(st[-1]["summed"].double().reshape(state["summed"].shape), state["summed"])

    ws = weights(spec, 6, grid=False)
    runs, runs0 = (plumbed(ws, lm, xs, times, watch, cast) for lm in (True, False))
    for (held, st, plan), (held0, st0, plan0) in zip(runs, runs0):
        assert held.keys() == held0.keys() and all(torch.equal(held[l], held0[l]) for l in held)
    assert_same_bits([([], st, plan) for _, st, plan in runs], [([], st, plan) for _, st, plan in runs0])
    assert sum(int(st[-1]["s"].sum()) for _, st, _ in runs0) > 0


def test_a_recording_handed_out_is_not_written_again():
    """What get("s") returned after one run still holds that run's train after the next."""
    from bindsnet_amd.network.monitors import Monitor
    spec, B = PLUMB
    net = build(spec, weights(spec, 5, grid=True, num=PLUMB_NUM), B, True).to("cuda")
    mons = {l: Monitor(net.layers[l], ["s"], time=7) for l in ("1", "3")}
    for l, m in mons.items():
        net.add_monitor(m, "m" + l)
    xs = [spike_input(spec, 7, B, 20 + i).to("cuda") for i in range(2)]
    net.run({"0": xs[0]}, time=7)
    held = {l: m.get("s") for l, m in mons.items()}
    first = {l: t.clone() for l, t in held.items()}
    net.run({"0": xs[1]}, time=7)
    assert net.last_plan == "layer-major"
    for l in held:
        assert torch.equal(held[l], first[l]) and not torch.equal(mons[l].get("s"), first[l]), f"layer {l}"


# ---- graphs and runs that do not qualify

REFUSED = (((3, 5, 5), [("conv", 5, 3, 1, 1), ("fc", 4)]), 5, 2)                  # (spec, T, B)


def _dense(net, src, dst, **kw):
    from bindsnet_amd.network.topology import Connection
    g = torch.Generator().manual_seed(3)
    a, b = net.layers[src], net.layers[dst]
    net.add_connection(Connection(a, b, w=torch.randn(a.n, b.n, generator=g) * 0.3, b=torch.full((b.n,), 0.3), **kw), src, dst)


def _sif(net, name, n=4, **kw):
    from bindsnet_amd.conversion import SubtractiveResetIFNodes
    net.add_layer(SubtractiveResetIFNodes(shape=(n,), thresh=1.0, reset=0.0, **kw), name)


def with_maxpool(net):
    from bindsnet_amd.conversion import PassThroughNodes
    from bindsnet_amd.network.topology import MaxPool2dConnection
    src = net.layers["1"]
    net.add_layer(PassThroughNodes(shape=(src.shape[0], src.shape[1] // 2, src.shape[2] // 2)), "3")
    net.add_connection(MaxPool2dConnection(src, net.layers["3"], kernel_size=2, stride=2, decay=1), "1", "3")


def with_v_monitor(net):
    from bindsnet_amd.network.monitors import Monitor
    net.add_monitor(Monitor(net.layers["1"], ["v"], time=REFUSED[1]), "v1")


def with_a_learning_rule(net):
    from bindsnet_amd.learning import PostPre
    _dense(net, "1", "2", update_rule=PostPre, nu=(1e-2, 1e-2))      # (in place of the chain's own "1" -> "2")


def with_norm(net):
    _dense(net, "1", "2", norm=2.0)


def with_two_feeders(net):
    from bindsnet_amd.network.nodes import Input
    net.add_layer(Input(shape=(6,)), "9")
    _dense(net, "9", "2")


def with_a_recurrent_connection(net):
    _sif(net, "3")
    _dense(net, "3", "3")                                            # its source is the layer itself: not yet walked


def with_a_source_further_on(net):
    _sif(net, "3")
    _sif(net, "4")
    _dense(net, "4", "3")                                            # "3" reads a layer that comes behind it
    _dense(net, "2", "4")


def with_another_node_type(net):
    from bindsnet_amd.network.nodes import IFNodes
    net.add_layer(IFNodes(shape=(4,), thresh=1.0, reset=0.0), "3")
    _dense(net, "2", "3")


def with_per_neuron_traces(net):
    _sif(net, "3", traces=True, tc_trace=torch.linspace(5.0, 20.0, 4))
    _dense(net, "2", "3")


def with_a_connection_monitor(net):
    from bindsnet_amd.network.monitors import Monitor
    net.add_monitor(Monitor(net.connections[("1", "2")], ["w"], time=REFUSED[1]), "w12")


class NoReward:
    def compute(self, **kwargs):
        return torch.tensor(0.0)

    def update(self, **kwargs):
        pass


def with_a_reward_fn(net):
    net.reward_fn = NoReward()


def as_it_is(net):
    pass


# name: (what is done to the chain, keyword arguments of build, keyword arguments of run)
REFUSALS = {
    "with_maxpool": (with_maxpool, {}, {}),
    "with_v_monitor": (with_v_monitor, {}, {}),
    "learning_rule": (with_a_learning_rule, {}, {}),
    "norm": (with_norm, {}, {}),
    "two_feeders": (with_two_feeders, {}, {}),
    "recurrent": (with_a_recurrent_connection, {}, {}),
    "source_further_on": (with_a_source_further_on, {}, {}),
    "another_node_type": (with_another_node_type, {}, {}),
    "input_traces": (as_it_is, dict(input_traces=True), {}),
    "per_neuron_traces": (with_per_neuron_traces, {}, {}),
    "connection_monitor": (with_a_connection_monitor, {}, {}),
    "one_step": (as_it_is, {}, dict(one_step=True)),
    "reward_fn": (with_a_reward_fn, {}, {}),
}


def refusal_twin(lm, extra, build_kw, run_kw):
    spec, T, B = REFUSED
    net = build(spec, weights(spec, 6, grid=False), B, lm, traces=True, extra=extra, **build_kw).to("cuda")
    inputs = {"0": spike_input(spec, T, B, 11).to("cuda")}
    if "9" in net.layers:
        inputs["9"] = (torch.rand(T, B, 6, generator=torch.Generator().manual_seed(4)) < 0.4).to(torch.uint8).to("cuda")
    net.run(inputs, time=T, **run_kw)
    bits = {}
    for l, layer in net.layers.items():
        for k in ("s", "v", "x", "refrac_count"):
            if isinstance(getattr(layer, k, None), torch.Tensor):
                bits[l + "." + k] = getattr(layer, k).detach().float().cpu().numpy().view(np.uint32)
    for key, conn in net.connections.items():
        if isinstance(getattr(conn, "w", None), torch.Tensor):
            bits["w" + "".join(key)] = conn.w.detach().float().cpu().numpy().view(np.uint32)
    return net.last_plan, bits


def test_the_chain_the_refusals_start_from_qualifies():
    assert refusal_twin(True, as_it_is, {}, {})[0] == "layer-major"


@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_graph_that_does_not_qualify_runs_the_generic_plan(name):
    """One clause of layer_major._chain (or of run's pre-check) each, added to a chain that qualifies (the test above): the twin that
    asks and the twin that does not report the same plan, not "layer-major", and leave the same bits in every layer's s, v, x and
    refrac_count and in every connection's w.
    Not built, because the public API does not reach them: `_pipe`, `_shard_state` and `_defer_norm` (set by bindsnet_amd.parallel
    and the pipelined run while they own the network); a non-float32 or non-contiguous `w` (Connection refuses another w_dtype when it
    is constructed, and the generic plan refuses a Conv2dConnection's half `w`, so there is no twin to compare with); a connection
    class outside the three, which every other clause above already needs a layer for (max-pool is the one built); B beyond
    MAX_OPERATOR_BATCH and a train beyond TRAIN_BUDGET_BYTES (sizes no quick test has); run's own keyword arguments (clamp, masks,
    ...: the same `kwargs` clause that `reward_fn` fills); an input that is too short or of another dtype or size, where the generic
    plan raises."""
    extra, build_kw, run_kw = REFUSALS[name]
    (plan, bits), (plan0, bits0) = (refusal_twin(lm, extra, build_kw, run_kw) for lm in (True, False))
    assert plan == plan0 and plan is not None and plan != "layer-major"
    if name in ("with_maxpool", "with_v_monitor", "another_node_type", "connection_monitor"):
        assert plan == "generic"
    assert bits.keys() == bits0.keys()
    for key in bits:
        assert np.array_equal(bits[key], bits0[key]), key
    assert sum(int((bits0[l + ".s"] != 0).sum()) + int((bits0[l + ".v"] != 0).sum()) for l in ("1", "2")) > 0


def test_a_converted_cnn_that_asks_runs_layer_major():
    """ann_to_snn(Conv-BN-ReLU-AvgPool-Flatten-Linear, layer_major=True) qualifies and gives what layer_major=False gives, bit for bit."""
    from bindsnet_amd.conversion import ann_to_snn
    from bindsnet_amd.network.monitors import Monitor
    torch.manual_seed(7)
    ann = torch.nn.Sequential(torch.nn.Conv2d(3, 6, 3, padding=1), torch.nn.BatchNorm2d(6), torch.nn.ReLU(), torch.nn.AvgPool2d(2),
                              torch.nn.Flatten(), torch.nn.Linear(6 * 4 * 4, 5)).eval()
    with torch.no_grad():
        ann[1].running_mean.uniform_(-0.2, 0.2), ann[1].running_var.uniform_(0.5, 1.5), ann[1].weight.uniform_(0.5, 1.5)
    T, B = 6, 2
    x = (torch.rand(T, B, 3, 8, 8, generator=torch.Generator().manual_seed(8)) < 0.4).to(torch.uint8).to("cuda")
    seen = []
    for lm in (True, False):
        snn = ann_to_snn(ann, input_shape=(3, 8, 8), data=torch.rand(16, 3, 8, 8, generator=torch.Generator().manual_seed(9)), layer_major=lm)
        snn = snn.to("cuda")
        names = [l for l in snn.layers if l != "Input"]
        for l in names:
            snn.add_monitor(Monitor(snn.layers[l], ["s"], time=T), "m" + l)
        snn.run({"Input": x}, time=T)
        seen.append((snn.last_plan, {l: snn.monitors["m" + l].get("s").to(torch.uint8).cpu() for l in names},
                     {l: snn.layers[l].v.float().cpu().numpy().view(np.uint32) for l in names}))
    assert (seen[0][0], seen[1][0]) == ("layer-major", "generic")
    for l in seen[0][1]:
        assert torch.equal(seen[0][1][l], seen[1][1][l]) and np.array_equal(seen[0][2][l], seen[1][2][l]), l
    assert sum(int(t.sum()) for t in seen[1][1].values()) > 0
