"""bindsnet.conversion on the MI355X.

* Every fixture case of tests/golden/make_golden_conversion.py (tests/conversion_cases.py) through Network.run on the device, on the
  generic plan (the only plan such a graph takes), in training mode.  Dyadic family: every field against the REFERENCE's record, bit
  for bit.  Float family: every field against the stated order (conversion_cases.stated_run: dense sums over the spiking sources
  ascending, bias last; torch's conv2d and max_pool2d) bit for bit -- tests/test_conversion_host.py holds the stated order to the
  reference --, and against the reference's record within the fixture's measured spreads.
* The step kernel by hand (ops.sif_step) against the stated order at N = 1, 255, 257, 600 x B = 1, 3, state and outputs in front of
  guard elements; ops.prop_gather and ops.pass_step against torch; compute() / forward() on device tensors.
* Two half runs, reset_state_variables(), pickling, network.to("cuda"), a voltage monitor step by step, clamp / unclamp on a
  PassThroughNodes layer, and every refusal, each before any state changes."""
import io
import itertools
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conversion_cases as CC
from test_conversion_host import _bits, _ns, check_snapshots, gold, params_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _built(name):
    g = gold(name)
    return g, CC.build(_ns(), name, params=params_of(name, g), seed=int(g["seed"])).to(DEV)


def _equal_snapshots(got, want, what):
    assert len(got) == len(want)
    for r, (a, b) in enumerate(zip(got, want)):
        for k, v in a.items():
            ref = np.asarray(b[k]).reshape(np.asarray(v).shape)
            if k.endswith("_raster"):
                assert np.array_equal(v, ref), f"{what} input {r}: {k} differs ({int(v.sum())} vs {int(ref.sum())} spikes)"
            else:
                x, y = _bits(v), _bits(ref)
                assert np.array_equal(x, y), f"{what} input {r}: {k} differs at {np.flatnonzero(x != y)[:5]}"


@pytest.mark.parametrize("name", CC.CASES)
def test_device_reproduces_fixture(name):
    g, net = _built(name)
    for l in net.layers.values():
        assert l.s.is_cuda and (not getattr(l, "sum_input", False) or l.summed.is_cuda)       # network.to("cuda") moved `summed`
    snaps = CC.run_case(_ns(), net, name, device=DEV)
    assert net.last_plan == "generic"
    assert all(int(v.sum()) > 0 for s in snaps for k, v in s.items() if k.endswith("_raster")), "an empty raster: the kernels were not reached"
    check_snapshots(name, snaps, g)                       # dyadic: bit for bit; float: rasters, refrac_count, traces exact, v and summed within the spreads
    if name in CC.FLOAT:                                  # half 1: the stated order, every field and the per-step voltages, bit for bit
        stated = [{k: v for k, v in s.items() if not k.endswith("_margin")} for s in CC.stated_run(name, params=params_of(name, g), seed=int(g["seed"]))]
        _equal_snapshots(snaps, stated, name)


@pytest.mark.parametrize("name", ["g_pad_spiking", "g_perm_0312", "mlp_fl_b3", "cnn_dy", "step_n257", "step_n600"])
def test_two_halves_equal_one_whole_run_on_the_device(name):
    g, net = _built(name)
    check_snapshots(name, CC.run_case(_ns(), net, name, device=DEV, halves=True, count=1), g)
    assert net.last_plan == "generic"


@pytest.mark.parametrize("name", ["step_n255", "mlp_dy_b3", "cnn_fl"])
def test_voltage_monitor_step_by_step(name):
    g, net = _built(name)
    snaps = CC.run_case(_ns(), net, name, device=DEV, count=1)
    stated = CC.stated_run(name, params=params_of(name, g), seed=int(g["seed"]), count=1)
    keys = [k for k in snaps[0] if k.endswith("_vrec")]
    assert keys
    for k in keys:
        assert np.array_equal(_bits(snaps[0][k]), _bits(stated[0][k])), k


# ---- the kernels by hand ------------------------------------------------------------------------------------------------------

GUARD = 64


def _guarded(t, fill):
    """`t` on the device in front of and behind GUARD elements of `fill`: (view, whole buffer)."""
    flat = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype, device=DEV)
    flat[GUARD:GUARD + t.numel()] = t.reshape(-1).to(DEV)
    return flat[GUARD:GUARD + t.numel()].view(t.shape), flat


def _guards_intact(flat, fill):
    return bool((flat[:GUARD] == fill).all()) and bool((flat[-GUARD:] == fill).all())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 255, 257, 600])
def test_sif_step_by_hand(N, B):
    from bindsnet_amd import _lib, ops
    rng = np.random.default_rng(100 * N + B)
    T = 10
    cur = torch.from_numpy((rng.random((T, B, N)) * 3 - 1.2).astype(np.float32))
    cur[0], cur[1] = 1.5, -0.25                       # every neuron spikes, then none does
    pervec = N in (257, 600)
    scale = torch.linspace(0.5, 1.5, N) if pervec else 0.75
    decay = float(torch.exp(-torch.tensor(0.5) / torch.tensor(8.0)))
    p = _lib.LifParams()
    p.thresh, p.refrac, p.dt, p.has_lbound, p.lbound = 1.0, 1.0, 0.5, 1, -0.5
    p.traces, p.traces_additive, p.trace_decay, p.trace_scale = 1, int(pervec), decay, 0.0 if pervec else 0.75
    v, vf = _guarded(torch.zeros(B, N), 9.0)
    rc, rcf = _guarded(torch.zeros(B, N), 9.0)
    x, xf = _guarded(torch.zeros(B, N), 9.0)
    sm, smf = _guarded(torch.zeros(B, N), 9.0)
    s, sf = _guarded(torch.zeros(B, N, dtype=torch.uint8), 9)
    rs, rsf = _guarded(torch.zeros(B, N, dtype=torch.uint8), 9)
    rv, rvf = _guarded(torch.zeros(B, N), 9.0)
    st = dict(v=np.zeros((B, N), np.float32), rc=np.zeros((B, N), np.float32))
    xs, sums = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
    pv = {"trace_scale": scale.to(DEV)} if pervec else None
    for t in range(T):
        ops.sif_step(v, rc, s, x, cur[t].to(DEV).contiguous(), p, summed=sm if t % 2 == 0 or N != 255 else None, raster_s=rs, raster_v=rv, pv=pv)
        spikes, _ = CC.sif_stated(st, cur[t].numpy(), 1.0, 1.0, 0.5, -0.5)
        xs = xs * np.float32(decay)
        if pervec:
            xs = xs + scale.numpy() * spikes.astype(np.float32)
        else:
            xs[spikes != 0] = np.float32(0.75)
        if t % 2 == 0 or N != 255:                     # (N = 255: `summed` is null every other step -- the instance without it)
            sums = sums + cur[t].numpy()
        assert np.array_equal(s.cpu().numpy(), spikes) and np.array_equal(rs.cpu().numpy(), spikes), t
        for got, want, what in ((v, st["v"], "v"), (rc, st["rc"], "refrac_count"), (x, xs, "x"), (sm, sums, "summed"), (rv, st["v"], "raster_v")):
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (t, what)
        if t == 0:
            assert spikes.all()
        if t == 1:
            assert not spikes.any()
    for flat, fill in ((vf, 9.0), (rcf, 9.0), (xf, 9.0), (smf, 9.0), (sf, 9), (rsf, 9), (rvf, 9.0)):
        assert _guards_intact(flat, fill), "a step wrote outside its tensors"


def test_gather_and_pass_by_hand():
    from bindsnet_amd import ops
    gen = torch.Generator().manual_seed(21)
    for shape in ((2, 3, 5), (7,), (3, 4), (40, 30, 20)):          # (the last: more than one workgroup per sample, 24000 outputs)
        s = torch.rand(3, *shape, generator=gen) < 0.5
        for dims in itertools.permutations(range(len(shape))):
            arrays, out_shape = ops.permute_geometry(shape, dims)
            want = s.permute(0, *[d + 1 for d in dims]).float()
            out, flat = _guarded(torch.zeros(3, *out_shape), 9.0)
            ops.prop_gather(s.to(DEV).contiguous(), out, arrays)
            assert torch.equal(out.cpu(), want) and _guards_intact(flat, 9.0), (shape, dims)
            prev = torch.rand(3, *out_shape, generator=gen)
            out[:] = prev.to(DEV)
            ops.prop_gather(s.to(DEV).contiguous(), out, arrays, accumulate=True)
            assert torch.equal(out.cpu(), prev + want) and _guards_intact(flat, 9.0), (shape, dims, "accumulate")
    for shape, pad in (((2, 3, 5), (1, 2, 2, 1)), ((2, 3, 5), (0, 0, 0, 0)), ((4, 6), (3, 0, 0, 2)), ((3, 50, 70), (5, 4, 3, 2))):
        s = torch.rand(2, *shape, generator=gen) < 0.6
        lead = (0,) * (len(shape) - 2)
        arrays, out_shape = ops.pad_geometry(shape, lead + (pad[2], pad[0]), lead + (pad[3], pad[1]))
        want = F.pad(s, pad).float()
        out, flat = _guarded(torch.full((2, *out_shape), 5.0), 9.0)
        ops.prop_gather(s.to(DEV).contiguous(), out, arrays)
        assert torch.equal(out.cpu(), want) and _guards_intact(flat, 9.0), (shape, pad)
    cur = torch.tensor([[0.0, 1.0, -0.0, 2.0, 1.0, 0.0, 1.0]])
    sp, flat = _guarded(torch.full((1, 7), 7, dtype=torch.uint8), 9)
    ops.pass_step(sp, cur.to(DEV))
    assert sp.cpu().tolist() == [[0, 1, 0, 1, 1, 0, 1]] and _guards_intact(flat, 9)
    with pytest.raises(Exception):                                  # a geometry that could read outside the source: refused by the library
        arrays, out_shape = ops.permute_geometry((2, 3, 5), (2, 0, 1))
        ops.prop_gather(torch.zeros(1, 29, dtype=torch.uint8, device=DEV), torch.zeros(1, 30, device=DEV), arrays)


def test_forward_and_compute_on_device_tensors():
    from bindsnet_amd.conversion import ConstantPad2dConnection, PassThroughNodes, PermuteConnection, SubtractiveResetIFNodes
    from bindsnet_amd.network import Network, nodes
    net = Network(dt=1.0, batch_size=2)
    X, P = nodes.Input(shape=(2, 3, 5)), PassThroughNodes(shape=[5, 2, 3])
    Y = SubtractiveResetIFNodes(n=4, thresh=1.0, reset=0.0, refrac=0, sum_input=True, traces=True)
    for name, l in (("X", X), ("P", P), ("Y", Y)):
        net.add_layer(l, name=name)
    perm = PermuteConnection(X, P, dims=(0, 3, 1, 2))
    net.add_connection(perm, "X", "P")
    net.to(DEV)
    s = (torch.rand(2, 2, 3, 5) < 0.5).to(DEV)
    out = perm.compute(s)
    assert out.is_cuda and torch.equal(out, s.permute(0, 3, 1, 2).float())
    pad = ConstantPad2dConnection(X, PassThroughNodes(shape=[2, 6, 8]), padding=(1, 2, 2, 1))
    assert torch.equal(pad.compute(s), F.pad(s, (1, 2, 2, 1)).float())
    P.forward(out)
    assert P.s.dtype == torch.bool and P.s.shape == (2, 5, 2, 3) and torch.equal(P.s, out != 0) and not P.v.any()
    cur = torch.tensor([[1.5, 0.5, -1.0, 1.0], [0.25, 2.0, 0.0, 0.75]], device=DEV)
    Y.forward(cur)
    assert Y.s.tolist() == [[True, False, False, True], [False, True, False, False]]
    assert Y.v.tolist() == [[0.5, 0.5, -1.0, 0.0], [0.25, 1.0, 0.0, 0.75]] and torch.equal(Y.summed, cur)
    assert torch.equal(Y.x, Y.s.float())
    with pytest.raises(NotImplementedError, match="analog"):
        perm.compute(s.float())


def test_pickle_and_reset_on_the_device():
    g, net = _built("mlp_dy_b3")
    ns = _ns()
    first = CC.run_case(ns, net, "mlp_dy_b3", device=DEV, count=1)           # (ends with reset_state_variables())
    x = CC.case_inputs("mlp_dy_b3", 0)["Input"].to(DEV)
    net.run({"Input": x}, time=60)
    last = list(net.layers.values())[-1]
    assert np.array_equal(_bits(last.summed.cpu().numpy()), _bits(first[0]["5_summed"])), "the same input behind a reset gives the same readout"
    buf = io.BytesIO()
    pickle.dump(net, buf)
    buf.seek(0)
    back = pickle.load(buf)
    kept = list(back.layers.values())[-1]
    assert kept.summed.is_cuda and torch.equal(kept.summed, last.summed) and float(last.summed.abs().sum()) > 0
    net.reset_state_variables()
    assert not last.summed.any() and not last.v.any() and not last.refrac_count.any() and not last.s.any()


def test_clamp_and_unclamp_on_a_pass_through_layer():
    """clamp / unclamp apply behind the layer's own step, as for IFNodes: the layer's spike monitor shows them, and the layer behind
    it is driven by them one step later."""
    name = "g_pad_1221"
    g, net = _built(name)
    ns = _ns()
    P, Y = net.layers["P"], net.layers["Y"]
    mon = ns.Monitor(P, ["s"], time=CC.GATHER_T)
    net.add_monitor(mon, name="P_s")
    x = CC.case_inputs(name, 0)["X"]
    clamp, unclamp = torch.zeros(P.n, dtype=torch.bool), torch.zeros(P.n, dtype=torch.bool)
    clamp[0], unclamp[1:P.n:2] = True, True                          # (element 0 is padding: always 0 unless clamped)
    net.run({"X": x.to(DEV)}, time=CC.GATHER_T, clamp={"P": clamp}, unclamp={"P": unclamp})
    assert net.last_plan == "generic"
    seen = torch.cat((torch.zeros_like(x[:1]), x[:-1]))              # P's input at step t: X's spikes of step t - 1
    want = F.pad(seen.reshape(CC.GATHER_T, CC.GATHER_B, 2, 3, 5), (1, 2, 2, 1)).reshape(CC.GATHER_T, CC.GATHER_B, -1).bool()
    want[:, :, clamp] = True
    want[:, :, unclamp] = False
    got = mon.get("s").cpu().reshape(CC.GATHER_T, CC.GATHER_B, -1)
    assert got.dtype == torch.bool and torch.equal(got, want) and bool(got[:, :, 0].all())
    wh, bh, wy, by = CC.gather_weights(name)
    summed = np.zeros((CC.GATHER_B, CC.GATHER_OUT), np.float32)
    prev = np.zeros((CC.GATHER_B, P.n), np.uint8)
    for t in range(CC.GATHER_T):                                      # Y's input at step t: P's spikes of step t - 1
        summed = summed + CC.dense_stated(prev, wy, by)
        prev = want[t].numpy().astype(np.uint8)
    assert np.array_equal(_bits(Y.summed.cpu().numpy()), _bits(summed))


# ---- refusals: each raises the named type before any state changes --------------------------------------------------------------

def _state_of(net):
    out = []
    for l in net.layers.values():
        for k in ("v", "refrac_count", "x", "summed"):
            t = getattr(l, k, None)
            if isinstance(t, torch.Tensor):
                out.append(t.detach().clone())
    for c in net.connections.values():
        if hasattr(c, "firing_rates"):
            out.append(c.firing_rates.detach().clone())
    return out, torch.get_rng_state()


def _refused(net, exc, match, **run):
    before, rng = _state_of(net)
    with pytest.raises(exc, match=match):
        net.run(**run)
    after, rng2 = _state_of(net)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and torch.equal(rng, rng2), "a refused run changed state"


def _gather_net(conn_of, src=(2, 3, 5), out=(5, 2, 3), extra=None):
    ns = _ns()
    net = ns.Network(dt=1.0, batch_size=2)
    net.add_layer(ns.Input(shape=src, traces=True), name="X")
    net.add_layer(ns.Pass(shape=list(out)), name="P")
    net.add_layer(ns.SIF(n=4, thresh=1.0, reset=0.0, refrac=0, sum_input=True), name="Y")
    net.add_connection(conn_of(ns, net.layers["X"], net.layers["P"]), "X", "P")
    net.add_connection(ns.Connection(net.layers["P"], net.layers["Y"], w=torch.ones(int(np.prod(out)), 4) / 8), "P", "Y")
    if extra is not None:
        extra(ns, net)
    return net.to(DEV)


def test_refusals_on_the_device():
    from bindsnet_amd.network import nodes, topology
    x = (torch.rand(3, 2, 2, 3, 5) < 0.5).byte().to(DEV)
    run = dict(inputs={"X": x}, time=3)
    perm = lambda dims: (lambda ns, a, b: ns.PermuteConnection(a, b, dims=dims))          # noqa: E731
    pad = lambda p: (lambda ns, a, b: ns.PadConnection(a, b, padding=p))                  # noqa: E731
    _refused(_gather_net(perm((0, 2, 3, 1))), RuntimeError, "shape", **run)               # permuted (3, 5, 2) is not the target's
    _refused(_gather_net(perm((1, 0, 2, 3))), NotImplementedError, "dims", **run)
    _refused(_gather_net(pad((1, -1, 0, 0)), out=(2, 3, 5)), NotImplementedError, "negative", **run)
    _refused(_gather_net(pad((1, 1, 1, 1)), out=(2, 3, 5)), RuntimeError, "shape", **run)
    _refused(_gather_net(pad((1, 1)), out=(2, 3, 7)), NotImplementedError, "4-tuple", **run)
    x4 = (torch.rand(3, 2, 2, 2, 2, 2) < 0.5).byte().to(DEV)
    _refused(_gather_net(perm((0, 1, 2, 3, 4)), src=(2, 2, 2, 2), out=(2, 2, 2, 2)), NotImplementedError, "dimensions", inputs={"X": x4}, time=3)
    # PassThroughNodes: another connection class, a second feeder, an external current, injects_v
    dense = lambda ns, a, b: ns.Connection(a, b, w=torch.ones(30, 30))                    # noqa: E731
    _refused(_gather_net(dense), NotImplementedError, "Connection into PassThroughNodes", **run)
    second = lambda ns, net: net.add_connection(ns.PermuteConnection(net.layers["X"], net.layers["P"], dims=(0, 3, 1, 2)), "X2", "P")   # noqa: E731
    _refused(_gather_net(perm((0, 3, 1, 2)), extra=second), NotImplementedError, "exactly one", **run)
    good = _gather_net(perm((0, 3, 1, 2)))
    _refused(good, NotImplementedError, "external current", inputs={"X": x, "P": torch.zeros(3, 2, 30, device=DEV)}, time=3)
    _refused(good, NotImplementedError, "injects_v", injects_v={"P": torch.ones(30)}, **run)
    _refused(good, NotImplementedError, "mask", masks={("X", "P"): torch.ones(30, 30)}, **run)
    good.add_monitor(_ns().Monitor(good.layers["P"], ["v"], time=3), name="Pv")
    _refused(good, NotImplementedError, "monitoring 'v'", **run)
    del good.monitors["Pv"]
    good.add_monitor(_ns().Monitor(good.layers["Y"], ["summed"], time=3), name="Ys")
    _refused(good, NotImplementedError, "summed", **run)
    del good.monitors["Ys"]
    good.add_monitor(_ns().Monitor(good.connections[("X", "P")], ["dims"], time=3), name="c")
    _refused(good, NotImplementedError, "monitor", **run)
    del good.monitors["c"]
    good.run(**run)                                                                       # ... and the graph itself runs
    assert good.last_plan == "generic" and float(good.layers["Y"].summed.abs().sum()) > 0
    # tensor-valued parameters, by name
    for pname, value in (("thresh", torch.ones(4)), ("reset", torch.zeros(4)), ("refrac", torch.ones(4, dtype=torch.long))):
        net = _gather_net(perm((0, 3, 1, 2)))
        setattr(net.layers["Y"], pname, value.to(DEV))
        _refused(net, NotImplementedError, pname, **run)
    net = _gather_net(perm((0, 3, 1, 2)))
    net.layers["Y"].lbound = torch.zeros(4, device=DEV)
    _refused(net, NotImplementedError, "lbound", **run)
    # what ann_to_snn's quirks make: refused before the run
    import warnings
    from bindsnet_amd.conversion import ann_to_snn
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        nobias = ann_to_snn(nn.Sequential(nn.Conv2d(1, 4, 3, bias=False), nn.ReLU(), nn.Linear(144, 3)), (1, 8, 8)).to(DEV)
        padq = ann_to_snn(nn.Sequential(nn.ConstantPad2d((1, 2, 0, 0), 0), nn.Linear(66, 3)), (2, 3, 8)).to(DEV)
        other = lambda: ann_to_snn(nn.Sequential(nn.Linear(5, 4), nn.ReLU(), nn.Linear(4, 3)), (5,), node_type=nodes.IFNodes)      # noqa: E731
        with pytest.raises(NotImplementedError, match="sum_input"):
            other()
    _refused(nobias, RuntimeError, "bias", inputs={"Input": (torch.rand(3, 1, 1, 8, 8) < 0.5).byte().to(DEV)}, time=3)
    _refused(padq, RuntimeError, "shape", inputs={"Input": (torch.rand(3, 1, 2, 3, 8) < 0.5).byte().to(DEV)}, time=3)
    # float-valued (analog) input spikes
    _refused(_gather_net(perm((0, 3, 1, 2))), NotImplementedError, "uint8 or bool", inputs={"X": x.float()}, time=3)
