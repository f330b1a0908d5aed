"""snn_prop_dense_auto_f32 -- Connection.compute with its body (matrix cores or event-driven) chosen on the device per tile of 16
samples -- on the MI355X: the bits are those of snn_prop_dense_f32 and of the oracle's ordered sum whichever body runs, the counters
say which one ran, and Network.run on the generic plan computes the same rasters, state and learned weights with either."""
import numpy as np
import pytest
import torch

import oracle
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


class mode:
    """snn_set_dense_prop_mode for a block: 0 the cost rule, 1 always event-driven, 2 the matrix body wherever it is exact."""

    def __init__(self, m):
        self.m = m

    def __enter__(self):
        from bindsnet_amd import ops
        ops.set_dense_prop_mode(self.m)

    def __exit__(self, *exc):
        from bindsnet_amd import ops
        ops.set_dense_prop_mode(0)


def counters():
    return torch.zeros(2, dtype=torch.int32, device=DEV)


# (B, Nin, N, density, bias, accumulate): one dimension at a time around B = 17, Nin = 100, N = 65 -- tile tails (B), the partial round
# and the staged-chunk boundary at 1024 (Nin), column groups of 64 and the event kernel's single block (N) --, the densities at the
# largest shape, every bias / accumulate combination at one shape.
SWEEP = ([(B, 100, 65, 0.3, B % 2 == 0, B % 3 == 0) for B in (1, 15, 16, 17, 33)]
         + [(17, Nin, 65, 0.3, Nin % 2 == 1, Nin % 3 == 1) for Nin in (1, 15, 16, 17, 100, 1024, 1025, 1041)]
         + [(17, 1040, 65, 0.3, True, False), (33, 3088, 65, 0.3, False, True)]      # whole 16-byte pieces beyond a chunk: the census sweep
         + [(17, 100, N, 0.3, N % 2 == 0, N % 3 == 0) for N in (1, 63, 64, 65, 130)]
         + [(33, 1041, 130, d, True, True) for d in (0.0, 0.02, 0.3, 1.0)]
         + [(16, 1024, 64, 0.3, b, a) for b in (False, True) for a in (False, True)])

_REF = {}


def operands(case):
    """W (signed), s, bias, out0 and the oracle's ordered sum for a sweep case: computed once, shared by the modes, never written."""
    if case not in _REF:
        B, Nin, N, dens, bias, acc = case
        W = synth.uniform_f32(31, (Nin, N), -1.0, 1.0)
        s = synth.dense_spikes(32, (B, Nin), dens)
        b = synth.uniform_f32(33, (N,), -0.5, 0.5) if bias else None
        out0 = synth.uniform_f32(34, (B, N), -1.0, 1.0) if acc else np.zeros((B, N), np.float32)
        ref = out0.copy()
        oracle.prop_dense(W, s, bias=b, out=ref, accumulate=acc)
        for a in (W, s, out0, ref) + (() if b is None else (b,)):
            a.setflags(write=False)
        _REF[case] = (W, s, b, out0, ref)
    return _REF[case]


@pytest.mark.parametrize("m", (2, 0))
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "B{}-Nin{}-N{}-d{}-{}{}".format(c[0], c[1], c[2], c[3], "b" if c[4] else "", "a" if c[5] else ""))
def test_auto_is_bit_identical_to_prop_dense_and_the_ordered_sum(case, m):
    from bindsnet_amd import ops
    B, Nin, N, dens, bias, acc = case
    W, s, b, out0, ref = operands(case)
    dW, ds = torch.from_numpy(W.copy()).to(DEV), torch.from_numpy(s.copy()).to(DEV)
    db = None if b is None else torch.from_numpy(b.copy()).to(DEV)
    got, ev = torch.from_numpy(out0.copy()).to(DEV), torch.from_numpy(out0.copy()).to(DEV)
    cnt = counters()
    with mode(m):
        ops.prop_dense_auto(dW, ds, got, bias=db, accumulate=acc, counters=cnt)
    ops.prop_dense(dW, ds, ev, bias=db, accumulate=acc)
    np.testing.assert_array_equal(bits(got), bits(ev))
    np.testing.assert_array_equal(bits(got), bits(ref))
    mt, et = cnt.tolist()
    tiles = (B + 15) // 16
    assert mt + et == tiles
    if m == 2:                                  # every tile with a spike in it took the matrix body
        want = sum(int(s[t * 16:(t + 1) * 16].any()) for t in range(tiles))
        assert mt == want, (mt, et, want)


def test_mixed_batch_one_tile_silent():
    """B = 33 in mode 2: samples 0 .. 15 dense, 16 .. 31 silent, sample 32 dense -- the silent tile takes the event body."""
    from bindsnet_amd import ops
    B, Nin, N = 33, 1041, 130
    W = synth.uniform_f32(41, (Nin, N), -1.0, 1.0)
    s = synth.dense_spikes(42, (B, Nin), 0.4)
    s[16:32] = 0
    b = synth.uniform_f32(43, (N,), -0.5, 0.5)
    dW, ds, db = (torch.from_numpy(a).to(DEV) for a in (W, s, b))
    got, ev = torch.empty(B, N, device=DEV), torch.empty(B, N, device=DEV)
    cnt, flags = counters(), torch.full((3,), 7, dtype=torch.int32, device=DEV)
    with mode(2):
        ops.prop_dense_auto(dW, ds, got, bias=db, counters=cnt, flags=flags)
    ops.prop_dense(dW, ds, ev, bias=db)
    np.testing.assert_array_equal(bits(got), bits(ev))
    ref = np.zeros((B, N), np.float32)
    oracle.prop_dense(W, s, bias=b, out=ref, accumulate=False)
    np.testing.assert_array_equal(bits(got), bits(ref))
    assert cnt.tolist() == [2, 1] and flags.tolist() == [1, 0, 1]


def test_one_byte_of_2_sends_its_tile_to_the_event_body():
    from bindsnet_amd import ops
    B, Nin, N = 32, 1041, 130
    W = synth.uniform_f32(51, (Nin, N), -1.0, 1.0)
    s = synth.dense_spikes(52, (B, Nin), 0.5)
    s[21, 1040] = 2                              # the last byte of a row of the second tile
    dW, ds = torch.from_numpy(W).to(DEV), torch.from_numpy(s).to(DEV)
    got, ev = torch.empty(B, N, device=DEV), torch.empty(B, N, device=DEV)
    cnt, flags = counters(), torch.full((2,), 7, dtype=torch.int32, device=DEV)
    with mode(2):
        ops.prop_dense_auto(dW, ds, got, counters=cnt, flags=flags)
    ops.prop_dense(dW, ds, ev)
    np.testing.assert_array_equal(bits(got), bits(ev))
    assert cnt.tolist() == [1, 1] and flags.tolist() == [1, 0]


def test_counters_add_up():
    from bindsnet_amd import ops
    B, Nin, N = 33, 784, 100
    dW = torch.from_numpy(synth.uniform_f32(61, (Nin, N), -1.0, 1.0)).to(DEV)
    out = torch.empty(B, N, device=DEV)
    cnt = counters()
    calls = 0
    for m in (0, 1, 2):
        for k, dens in enumerate((0.0, 0.01, 0.06, 0.2, 0.9)):
            ds = torch.from_numpy(synth.dense_spikes(62 + k, (B, Nin), dens)).to(DEV)
            with mode(m):
                ops.prop_dense_auto(dW, ds, out, counters=cnt)
            calls += 1
            mt, et = cnt.tolist()
            assert mt + et == calls * 3
            if m == 1:
                assert mt == before_mt
            before_mt = mt
    ops.prop_dense_auto(dW, ds, out)            # counters are optional
    assert cnt.tolist() == [mt, et]


@pytest.mark.parametrize("dens,want", [(0.5, [1, 0]), (0.01, [0, 1])])
def test_the_rules_two_ends(dens, want):
    """B = 16, 1600 -> 256 under the cost rule: at 50 % the longest event walk is about 800 rows against 100 rounds of the chain, at 1 %
    about 16 -- several-fold margins on either side of any calibration (profiles/r06_dense_mfma_density_map.json)."""
    from bindsnet_amd import ops
    B, Nin, N = 16, 1600, 256
    dW = torch.from_numpy(synth.uniform_f32(71, (Nin, N), -1.0, 1.0)).to(DEV)
    s = synth.dense_spikes(72, (B, Nin), dens)
    ds = torch.from_numpy(s).to(DEV)
    got, ev = torch.empty(B, N, device=DEV), torch.empty(B, N, device=DEV)
    cnt = counters()
    for _ in range(3):                          # every tile-step, not one
        ops.prop_dense_auto(dW, ds, got, counters=cnt)
    ops.prop_dense(dW, ds, ev)
    np.testing.assert_array_equal(bits(got), bits(ev))
    assert cnt.tolist() == [3 * want[0], 3 * want[1]], (cnt.tolist(), int((s != 0).sum(1).max()))


# ---- Network.run on the generic plan -----------------------------------------------------------------------------------------------
T, B = 30, 17


def build(n_in=64, ask=False):
    from bindsnet_amd.learning import PostPre
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.monitors import Monitor
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Connection
    g = torch.Generator().manual_seed(5)
    net = Network(dt=1.0)
    net.add_layer(Input(n=n_in, traces=True), "X")
    net.add_layer(LIFNodes(n=48, traces=True), "H")
    net.add_layer(LIFNodes(n=32, traces=True), "Y")
    net.add_connection(Connection(net.layers["X"], net.layers["H"], w=torch.rand(n_in, 48, generator=g) * (51.2 / n_in),
                                  b=torch.rand(48, generator=g) - 0.5, prop_auto=ask), "X", "H")
    net.add_connection(Connection(net.layers["H"], net.layers["Y"], w=torch.rand(48, 32, generator=g) * 2.0, update_rule=PostPre,
                                  nu=(1e-3, 1e-2), reduction=torch.sum, wmin=0.0, wmax=2.0), "H", "Y")
    for name in ("H", "Y"):
        net.add_monitor(Monitor(net.layers[name], ["s"], time=T), name)
    return net


def run(m, pieces, n_in=64, ask=False):
    """The network's run over the T steps in `pieces` consecutive calls under dense-prop mode m: rasters, state, weights, stats."""
    inp = (np.random.default_rng(9).random((T, B, n_in)) < 0.4).astype(np.uint8)
    with mode(m):
        net = build(n_in, ask).to(DEV)
        ras = {"H": [], "Y": []}
        step = T // pieces
        for p in range(pieces):
            net.run({"X": torch.from_numpy(inp[p * step:(p + 1) * step]).to(DEV)}, time=step)
            assert net.last_plan == "generic"
            for name in ras:
                ras[name].append(net.monitors[name].get("s").cpu().numpy().reshape(-1, B, net.layers[name].n)[-step:].copy())
        out = {"s" + k: np.concatenate(v).astype(np.uint8) for k, v in ras.items()}
        for name in ("H", "Y"):
            out["v" + name] = net.layers[name].v.cpu().numpy().copy()
            out["x" + name] = net.layers[name].x.cpu().numpy().copy()
        out["xX"] = net.layers["X"].x.cpu().numpy().copy()
        out["w"] = net.connections[("H", "Y")].w.detach().cpu().numpy().copy()
        return out, net.prop_stats()


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = (v.view(np.uint32) if v.dtype == np.float32 else v for v in (a[k], b[k]))
        np.testing.assert_array_equal(x, y, err_msg=k)


def test_network_matrix_and_event_bodies_agree():
    mat, st_mat = run(2, 1)
    evt, st_evt = run(1, 1)
    assert mat["sH"].sum() > 0 and mat["sY"].sum() > 0 and not np.array_equal(mat["w"], build().connections[("H", "Y")].w.numpy())
    same(mat, evt)
    tiles = T * ((B + 15) // 16)
    for key in (("X", "H"), ("H", "Y")):
        assert st_evt[key] == {"matrix_tiles": 0, "event_tiles": tiles}
        assert st_mat[key]["matrix_tiles"] + st_mat[key]["event_tiles"] == tiles
    assert st_mat[("X", "H")]["matrix_tiles"] == tiles - 2       # (step 0 propagates the Input's initial, silent spikes)
    assert st_mat[("H", "Y")]["matrix_tiles"] > 0
    halves, st_half = run(2, 2)
    same(mat, halves)
    assert st_half == st_mat
    # under the rule nobody asked: every connection keeps the single event-driven launch, nothing is counted
    rule, st_rule = run(0, 1)
    same(mat, rule)
    assert all(v == {"matrix_tiles": 0, "event_tiles": 0} for v in st_rule.values())


def test_under_the_rule_only_a_connection_that_asks_and_has_256_sources_takes_the_choice():
    """Connection(prop_auto=True) with 256 sources: under the rule its 40 %-dense steps run on the matrix cores and the bits are those
    of the same network without the request, which counts nothing; with 64 sources the request changes nothing."""
    tiles = T * ((B + 15) // 16)
    plain, st_plain = run(0, 1, n_in=256)
    asked, st_asked = run(0, 1, n_in=256, ask=True)
    same(plain, asked)
    assert plain["sH"].sum() > 0 and plain["sY"].sum() > 0
    assert all(v == {"matrix_tiles": 0, "event_tiles": 0} for v in st_plain.values())
    assert st_asked[("X", "H")] == {"matrix_tiles": tiles - 2, "event_tiles": 2}      # (step 0: the Input's initial, silent spikes)
    assert st_asked[("H", "Y")] == {"matrix_tiles": 0, "event_tiles": 0}              # (never asked)
    small, st_small = run(0, 1, n_in=64, ask=True)
    assert all(v == {"matrix_tiles": 0, "event_tiles": 0} for v in st_small.values())
