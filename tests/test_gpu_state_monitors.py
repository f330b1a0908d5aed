"""State monitors on the MI355X: x, theta, refrac_count, i of layers and `activity` of MulticompartmentConnection(traces=True),
copied out at the end of every timestep by one launch (snn_record_segments, csrc/snn_ops.hip).

  * ops.record_segments against torch copies, compared as int32 bits: lengths around the 16-byte and the 4 KiB block boundaries,
    4-byte and 16-byte aligned ends, segment counts around the 32 of one launch, first and last slice, sentinels around every slice;
  * every reference-generated fixture of tests/state_monitor_cases.py on the device, generic plan, bit for bit (`activity`: equal,
    zeros of either sign) with the reference's generator state;
  * DiehlAndCook2015 with a theta / x monitor against the same seeded network without it, on whatever plan that takes;
  * a kept descriptor set never writes into a record an earlier get() handed out; sparse=True, time=None and a short window on x
    behave as they do for v."""
import numpy as np
import pytest
import torch

import state_monitor_cases as SC
from test_state_monitors_host import check_snapshots, ns

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025)
OFFSETS = ((0, 0), (0, 1), (1, 0), (1, 1))           # (source, destination) float offsets inside their allocations
SENTINEL = 0x5A5A5A5A
NAN_PAYLOAD = 0x7FC12345                             # a quiet NaN whose payload is not the default one
NEG_ZERO = -0x80000000                               # the bits of -0.0 as int32


@pytest.fixture(autouse=True)
def few_host_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(4, n))
    yield
    torch.set_num_threads(n)


def _segment(gen, n, T, src_off, dst_off):
    """A source of n floats at float offset src_off and a [T, n] destination at dst_off, both inside sentinel-filled allocations;
    random bits (NaNs of every kind among them), -0.0 first and a NaN with a payload last."""
    src_all = torch.full((n + src_off + 1,), SENTINEL, dtype=torch.int32)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    bits[0] = NEG_ZERO
    bits[-1] = NAN_PAYLOAD if n > 1 or T % 2 else NEG_ZERO
    src_all[src_off:src_off + n] = bits
    src_all = src_all.to(DEV)
    dst_all = torch.full((T * n + dst_off + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    src = src_all[src_off:src_off + n].view(torch.float32)
    dst = dst_all[dst_off:dst_off + T * n].view(torch.float32).view(T, n)
    assert src.data_ptr() % 16 == 4 * src_off and dst.data_ptr() % 16 == 4 * dst_off
    return src_all, dst_all, src, dst


def _check_call(specs, T, t, seed):
    """One ops.record_segments call over `specs` = [(n, src_off, dst_off)]; every destination allocation, sentinels included,
    against a torch copy of the int32 bits."""
    from bindsnet_amd import ops
    gen = torch.Generator().manual_seed(seed)
    segs = [_segment(gen, n, T, so, do) for n, so, do in specs]
    want = []
    for (n, so, do), (src_all, dst_all, src, dst) in zip(specs, segs):
        w = dst_all.clone()
        w[do + t * n:do + (t + 1) * n] = src_all[so:so + n]
        want.append(w)
    ops.record_segments([(src, dst) for _, _, src, dst in segs], t)
    torch.cuda.synchronize()
    for k, ((n, so, do), (src_all, dst_all, _, _), w) in enumerate(zip(specs, segs, want)):
        bad = torch.nonzero(dst_all != w).flatten()[:5].tolist()
        assert not bad, f"segment {k} (n = {n}, offsets {so}/{do}, t = {t}): int32 words {bad} differ"
        assert int(src_all[0]) == SENTINEL or so == 0, "source allocation overwritten"
        assert int(src_all[-1]) == SENTINEL, "source allocation overwritten"


@pytest.mark.parametrize("t", (0, 2))
def test_record_segments_lengths_and_alignments(t):
    """Every length at every pair of offsets in ONE call: 40 segments, so two launches (32 + 8)."""
    specs = [(n, so, do) for so, do in OFFSETS for n in LENGTHS]
    _check_call(specs, T=3, t=t, seed=11 + t)


@pytest.mark.parametrize("count", (1, 2, 31, 32, 33))
@pytest.mark.parametrize("t", (0, 2))
def test_record_segments_counts(count, t):
    specs = [(LENGTHS[(3 * k + count) % len(LENGTHS)], *OFFSETS[(k + count) % 4]) for k in range(count)]
    _check_call(specs, T=3, t=t, seed=100 + count)


@pytest.mark.parametrize("t", (0, 1))
def test_record_segments_many_blocks(t):
    """3 * 2^18 + 1 floats: 769 blocks of 4 KiB per segment, a one-word tail, at all four offset pairs."""
    n = 3 * 2 ** 18 + 1
    _check_call([(n, so, do) for so, do in OFFSETS], T=2, t=t, seed=7)


def test_record_segments_refuses_what_it_cannot_copy():
    from bindsnet_amd import ops
    src, dst = torch.zeros(6, device=DEV), torch.zeros(3, 6, device=DEV)
    for bad_t in (-1, 3):
        with pytest.raises(ValueError):
            ops.record_segments([(src, dst)], bad_t)
    with pytest.raises(ValueError):
        ops.record_segments([(src, torch.zeros(3, 5, device=DEV))], 0)
    with pytest.raises(TypeError):
        ops.record_segments([(src.double(), dst)], 0)
    ops.record_segments([], 0)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_device_reproduces_reference_fixture(name):
    n = ns()
    net = SC.build(n, name).to(DEV)
    snaps = SC.run_case(n, net, name, device=DEV)
    assert net.last_plan == "generic"
    check_snapshots(name, snaps)


def _dc2015(monitored):
    from bindsnet_amd import synth
    from bindsnet_amd.models import DiehlAndCook2015
    from bindsnet_amd.network.monitors import Monitor
    N, B, T = 100, 2, 30
    torch.manual_seed(0)
    net = DiehlAndCook2015(n_inpt=784, n_neurons=N, exc=22.5, inh=120, dt=1.0, norm=78.4, theta_plus=0.05, inpt_shape=(1, 28, 28))
    net.connections[("X", "Ae")].pipeline[0].value.data.copy_(torch.from_numpy(synth.weights_q12(10, 784, N)))
    mons = {k: Monitor(net.layers[k], ["s"], time=T) for k in ("Ae", "Ai")}
    if monitored:
        mons["state"] = Monitor(net.layers["Ae"], ["theta", "x"], time=T)
    for k, m in mons.items():
        net.add_monitor(m, k)
    net.to(DEV)
    x = torch.from_numpy(synth.spike_train(20, T, B, 784)).view(T, B, 1, 28, 28).to(DEV)
    torch.manual_seed(2)
    net.run({"X": x}, time=T)
    torch.cuda.synchronize()
    return net, mons


def test_diehl_and_cook_2015_with_a_theta_and_trace_monitor():
    plain, pm = _dc2015(False)
    net, m = _dc2015(True)
    assert net.last_plan == "generic", net.last_plan
    for k in ("Ae", "Ai"):
        a, b = pm[k].get("s").cpu(), m[k].get("s").cpu()
        assert torch.equal(a, b), f"{k} raster differs from the unmonitored run ({plain.last_plan})"
    assert int(m["Ae"].get("s").sum()) > 0, "vacuous"
    bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)      # noqa: E731
    for key in net.connections:
        for f0, f1 in zip(plain.connections[key].pipeline, net.connections[key].pipeline):
            assert torch.equal(bits(f0.value), bits(f1.value)), f"weights of {key} differ from the unmonitored run"
    Ae = net.layers["Ae"]
    assert torch.equal(bits(plain.layers["Ae"].theta), bits(Ae.theta)) and float(Ae.theta.max()) > 0
    theta, x = m["state"].get("theta"), m["state"].get("x")
    assert tuple(theta.shape) == (30, 100) and tuple(x.shape) == (30, 2, 100) and theta.dtype == x.dtype == torch.float32
    assert torch.equal(bits(theta[-1]), bits(Ae.theta)) and torch.equal(bits(x[-1]), bits(Ae.x))
    assert bool((theta[1:] >= theta[:-1] * 0.999).all()) and float(x.max()) > 0


def _small(T, monitors):
    """Case (a)'s network on the device with the given {name: (variables, Monitor keywords)}."""
    n = ns()
    net = SC.build(n, "a").to(DEV)
    mons = {k: n.Monitor(net.layers["Y"], list(vars_), **kw) for k, (vars_, kw) in monitors.items()}
    for k, m in mons.items():
        net.add_monitor(m, k)
    return net, mons


def test_a_kept_descriptor_set_never_overwrites_an_earlier_record():
    T = SC.CASES["a"]["T"]
    net, mons = _small(T, {"m": (("x", "theta", "refrac_count"), dict(time=T))})
    ints = lambda t: t.contiguous().view(torch.int32)      # noqa: E731
    net.run({"X": torch.from_numpy(SC.inputs("a", 0)).to(DEV)}, time=T)
    kept = net.__dict__["_run_cache"]
    assert kept is not None
    first = {v: mons["m"].get(v) for v in ("x", "theta", "refrac_count")}
    copies = {v: t.clone() for v, t in first.items()}
    net.run({"X": torch.from_numpy(SC.inputs("a", 1)).to(DEV)}, time=T)
    torch.cuda.synchronize()
    assert net.__dict__["_run_cache"] is kept, "the second run rebuilt the descriptors: the test does not exercise the kept set"
    assert net.last_plan == "generic"
    for v, t in first.items():
        assert torch.equal(ints(t), ints(copies[v])), f"the first run's record of {v} changed during the second run"
        second = mons["m"].get(v)
        assert second.data_ptr() != t.data_ptr() and tuple(second.shape) == tuple(t.shape)
        assert not torch.equal(ints(second), ints(t)), f"{v}: the second run recorded nothing new"
    assert torch.equal(ints(mons["m"].get("theta")[-1]), ints(net.layers["Y"].theta))


def test_sparse_unbounded_and_short_windows_on_x_behave_as_for_v():
    T = SC.CASES["a"]["T"]
    short = T // 4
    net, mons = _small(T, {"full": (("x", "v"), dict(time=T)), "sparse": (("x", "v"), dict(time=T, sparse=True)),
                           "grow": (("x", "v"), dict(time=None)), "short": (("x", "v"), dict(time=short))})
    net.run({"X": torch.from_numpy(SC.inputs("a", 0)).to(DEV)}, time=T)
    ints = lambda t: t.cpu().contiguous().view(torch.int32)      # noqa: E731
    full = {v: mons["full"].get(v) for v in ("x", "v")}
    assert float(full["x"].max()) > 0, "vacuous"
    for v in ("x", "v"):
        sp = mons["sparse"].get(v)
        assert sp.is_sparse and torch.equal(ints(sp.to_dense()), ints(full[v]))
        sh = mons["short"].get(v)
        assert tuple(sh.shape) == (short, *full[v].shape[1:]) and torch.equal(ints(sh), ints(full[v][-short:]))
        g = mons["grow"].get(v)
        assert torch.equal(ints(g), ints(full[v]))
        assert mons["grow"].recording[v] == [], "time=None: get() empties the record"
    net.run({"X": torch.from_numpy(SC.inputs("a", 1)).to(DEV)}, time=T)
    for v in ("x", "v"):
        g = mons["grow"].get(v)
        assert tuple(g.shape) == tuple(full[v].shape), "time=None: the second run's record alone"
        f2 = mons["full"].get(v)
        assert tuple(f2.shape) == tuple(full[v].shape) and torch.equal(ints(g), ints(f2))
        sh = mons["short"].get(v)
        assert torch.equal(ints(sh), ints(f2[-short:]))
    xs, vs = mons["sparse"].get("x"), mons["sparse"].get("v")
    assert xs.is_sparse == vs.is_sparse and xs.device == vs.device and xs.dtype == vs.dtype and xs.shape[0] == vs.shape[0]
