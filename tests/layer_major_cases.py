"""What the layer-major tests share: a chain network built from a short spec, its plain float64 reference, the GPU test's table of
cases and the kernel's geometry restated in Python, so that every case can say which branch of snn_run_conv2d_sif_f32 it is there for
and a test can assert that it still reaches it (tests/test_layer_major_cases.py on the host, tests/test_gpu_layer_major.py before a run).

A spec is (input shape, [("conv", cout, k | (kh, kw), stride, pad) | ("pool",) | ("fc", n)]).  `grid=True` puts every weight and bias
on a 1/64 grid with small integer numerators (threshold 1, 2x2 pooling, inputs 0 / 1 / 2 or multiples of 1/4): every partial sum is
then exact in float32 in any order (tests/conv_wide_cases.py's device), so the float64 result is the only correct one and equality is
exact.  The bound: every value is an integer over 64 * 4 = 256.  The largest sum is "stream_odd"'s, 49 * 7 * 7 = 2401 taps of at most
12 / 64 times a byte of at most 2, i.e. 2401 * 12 * 2 * 4 = 230 496 units per step; v and `summed` add at most ten such steps (two
runs of T = 5) and a bias of 8 / 64: below 2.4e6, far below 2^24 = 16.8e6.  Trace decays and scales are 0.5 and 1, entry traces
multiples of 1/64 in [0, 1] and T at most 7: x stays a multiple of 2^-13 below 2."""
import numpy as np
import torch
import torch.nn.functional as F


def khw(k):
    return (k, k) if isinstance(k, int) else tuple(k)


def shapes(spec):
    shape, out = tuple(spec[0]), []
    for op in spec[1]:
        if op[0] == "conv":
            _, cout, k, s, p = op
            kh, kw = khw(k)
            shape = (cout, (shape[1] + 2 * p - kh) // s + 1, (shape[2] + 2 * p - kw) // s + 1)
        elif op[0] == "pool":
            shape = (shape[0], shape[1] // 2, shape[2] // 2)
        else:
            shape = (op[1],)
        out.append(shape)
    return out


def weights(spec, seed, grid, num=(-4, 12)):
    """[(w, b) or None] per op: conv w [Cout, Cin, kh, kw], fc w [n_in, n_out].  `num`: the range of the grid's numerators, both ends
    included, or one range per op."""
    rng, prev, out = np.random.default_rng(seed), tuple(spec[0]), []
    nums = [num] * len(spec[1]) if isinstance(num[0], int) else list(num)
    for op, shape, lohi in zip(spec[1], shapes(spec), nums):
        lo, hi = lohi or (0, 0)                        # (a pool has no weights)
        if op[0] == "pool":
            out.append(None)
        else:
            wshape = (op[1], prev[0], *khw(op[2])) if op[0] == "conv" else (int(np.prod(prev)), op[1])
            fan = int(np.prod(wshape[1:])) if op[0] == "conv" else wshape[0]
            if grid:                                   # numerators in [-4, 12]: a mean of 4/64 per tap, about one threshold per 16 active taps
                w, b = rng.integers(lo, hi + 1, wshape) / 64.0, rng.integers(-8, 9, wshape[0] if op[0] == "conv" else wshape[1]) / 64.0
            else:
                w, b = rng.standard_normal(wshape) * 2.0 / np.sqrt(fan) + 0.5 / fan, rng.standard_normal(shape[0]) * 0.1
            out.append((torch.from_numpy(w.astype(np.float32)), torch.from_numpy(b.astype(np.float32))))
        prev = shape
    return out


def build(spec, ws, B, layer_major, refrac=0, lbound=None, traces=False, extra=None, input_traces=False, trace_decay=None):
    """The chain as a bindsnet_amd Network (on the host; the caller moves it).  The last layer has sum_input.  `trace_decay`: written over
    what the layers derived from tc_trace (e ^ (-dt / tc_trace) is not exact in binary; 0.5 is, and then so is every trace)."""
    from bindsnet_amd.conversion import SubtractiveResetIFNodes
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input
    from bindsnet_amd.network.topology import AvgPool2dConnection, Connection, Conv2dConnection
    net = Network(batch_size=B)
    net.layer_major = layer_major
    prev = Input(shape=spec[0], traces=input_traces)
    net.add_layer(prev, "0")
    for i, (op, shape, wb) in enumerate(zip(spec[1], shapes(spec), ws), start=1):
        layer = SubtractiveResetIFNodes(shape=shape, thresh=1.0, reset=0.0, refrac=refrac, lbound=lbound, traces=traces,
                                        sum_input=i == len(spec[1]))
        if op[0] == "conv":
            conn = Conv2dConnection(prev, layer, kernel_size=op[2], stride=op[3], padding=op[4], w=wb[0].clone(), b=wb[1].clone(), prop_auto=True)
        elif op[0] == "pool":
            conn = AvgPool2dConnection(prev, layer, kernel_size=2)
        else:
            conn = Connection(prev, layer, w=wb[0].clone(), b=wb[1].clone(), prop_auto=True)
        net.add_layer(layer, str(i))
        net.add_connection(conn, str(i - 1), str(i))
        if traces and trace_decay is not None:
            layer.trace_decay.fill_(trace_decay)
        prev = layer
    if extra is not None:
        extra(net)
    return net


def trace_next(x, s, decay, scale, additive):
    """snn_common.hpp's trace_next in float64: x * decay, then + scale * s (additive) or set to scale where s."""
    t = x * decay
    return t + scale * s if additive else torch.where(s > 0, torch.full_like(t, scale), t)


def if_step(v, rc, cur, refrac=0, lbound=None):
    """SubtractiveResetIFNodes.forward at threshold 1, dt 1 on float64 v and refrac_count, in place; returns the spikes (bool)."""
    v += (rc == 0).double() * cur
    rc.copy_((rc > 0).double() * (rc - 1.0))
    s = v >= 1.0
    rc[s] = float(refrac)
    v[s] -= 1.0
    if lbound is not None:
        v.clamp_(min=lbound)
    return s


def reference(spec, ws, x, state, refrac=0, lbound=None, traces=None, entry=None):
    """One run of the chain in float64, step by step: layer k at step t reads layer k-1's spikes of step t-1.  x [T, B, *shape]; `state`
    (a dict, {} before the first run) carries every layer's s, v, refrac_count, x (the trace) and the last layer's summed from run to
    run.  `traces`: None or (decay, scale, additive).  `entry`: the state before the first run where that is not zero, a dict of lists
    like `state` (any of s, v, rc, x, summed; float64, the layers' shapes with the batch in front).  Returns the trains [T, B, *shape]."""
    T, B = x.shape[:2]
    n = len(spec[1])
    if not state:
        zeros = lambda: [torch.zeros(B, *sh, dtype=torch.float64) for sh in shapes(spec)]      # noqa: E731
        state.update(s=[torch.zeros(B, *spec[0], dtype=torch.float64)] + zeros(), v=zeros(), rc=zeros(), x=zeros(),
                     summed=torch.zeros(B, *shapes(spec)[-1], dtype=torch.float64))
        for key, val in (entry or {}).items():
            state[key] = val.double().clone() if isinstance(val, torch.Tensor) else [t.double().clone() for t in val]
    trains = [torch.zeros(T, B, *sh, dtype=torch.uint8) for sh in shapes(spec)]
    for t in range(T):
        prev = list(state["s"])
        state["s"][0] = x[t].double()
        for k, (op, wb) in enumerate(zip(spec[1], ws)):
            if op[0] == "conv":
                cur = F.conv2d(prev[k], wb[0].double(), wb[1].double(), stride=op[3], padding=op[4])
            elif op[0] == "pool":
                cur = F.avg_pool2d(prev[k], 2)
            else:
                cur = F.linear(prev[k].reshape(B, -1), wb[0].double().t(), wb[1].double())
            s = if_step(state["v"][k], state["rc"][k], cur, refrac, lbound)
            if traces is not None:
                state["x"][k] = trace_next(state["x"][k], s.double(), *traces)
            if k == n - 1:
                state["summed"] += cur
            state["s"][k + 1] = s.double()
            trains[k][t] = s.to(torch.uint8)
    return trains


def spike_input(spec, T, B, seed, density=0.3, analog=False):
    rng = np.random.default_rng(seed)
    if analog:                                         # multiples of 1/4 in [0, 1]: products with the 1/64 grid stay exact
        return torch.from_numpy((rng.integers(0, 5, (T, B, *spec[0])) / 4.0).astype(np.float32))
    return torch.from_numpy((rng.random((T, B, *spec[0])) < density).astype(np.uint8))


# ---- the geometry of snn_run_conv2d_sif_f32, restated from csrc/snn_conv_mfma.hpp, snn_conv_wide.hpp and snn_run_conv_sif.hpp

BLOCK_PIX, SLAB_ROWS, LDS_LIMIT, STAGE_WORDS = 64, 64, 150 * 1024, 8 * 256       # kBlockPix, kSlabRows, kLdsLimit, kStageRegs * threads


def padded_terms(cin, kh, kw):
    return kh * kw * ((cin + 15) // 16 * 16)


def slab_count(cin, kh, kw):
    return -(-padded_terms(cin, kh, kw) // SLAB_ROWS)


def wide_pixel_stride(cin):
    return (((cin + 15) // 16) | 1) * 16


def band_of(p0, g):
    """(iy0, rows): the input rows that output pixels p0 .. p0 + 63 of one sample read.  g: the dict of `geometry`."""
    hi = min(p0 + BLOCK_PIX - 1, g["OH"] * g["OW"] - 1)
    a = p0 // g["OW"] * g["stride"] - g["pad"]
    z = hi // g["OW"] * g["stride"] - g["pad"] + g["KH"] - 1
    iy0, iy1 = min(max(a, 0), g["H"]), min(z, g["H"] - 1)
    return iy0, max(iy1 - iy0 + 1, 0)


def band_words(g, rows):
    return rows * g["W"] * (wide_pixel_stride(g["Cin"]) // 4)


def geometry(spec, k=0):
    """What the kernel's plan makes of the spec's conv number k (its input must be the op before it): extents, blocks, slabs, the band
    words of every block, whether the bank stays resident, whether the stores are packed, the live tiles of the last block."""
    cin, H, W = tuple(spec[0]) if k == 0 else shapes(spec)[k - 1]
    _, cout, kk, stride, pad = spec[1][k]
    KH, KW = khw(kk)
    g = dict(Cin=cin, H=H, W=W, KH=KH, KW=KW, stride=stride, pad=pad, Cout=cout, OH=(H + 2 * pad - KH) // stride + 1, OW=(W + 2 * pad - KW) // stride + 1)
    nps = g["OH"] * g["OW"]
    g["nps"], g["blocks"], g["groups"], g["slabs"] = nps, -(-nps // BLOCK_PIX), -(-cout // 16), slab_count(cin, KH, KW)
    g["words"] = [band_words(g, band_of(p0, g)[1]) for p0 in range(0, nps, BLOCK_PIX)]
    span = min((g["OW"] + BLOCK_PIX - 2) // g["OW"] + 1, g["OH"])
    bands = 2 * max(16, min((span - 1) * stride + KH, H) * W * wide_pixel_stride(cin))
    g["resident"] = g["slabs"] * SLAB_ROWS * 16 * 4 + bands <= LDS_LIMIT
    g["packed"] = nps % 4 == 0
    g["last_live_tiles"] = -(-(nps - (g["blocks"] - 1) * BLOCK_PIX) // 16)
    g["last_group_channels"] = cout - (g["groups"] - 1) * 16
    return g


# ---- the cases of tests/test_gpu_layer_major.py
# name: (spec, T, B, options, what the first conv's geometry must be for the case to be worth its name).  Kernel 1 is every "conv" fed
# spike bytes; the shapes are the smallest at which it can go wrong.  Options: refrac, lbound, traces; density of the input; `two`:
# [(run, frame)] where one input byte is 2, so that the step which reads the frame takes the scalar body; `num`: the grid's numerators,
# chosen per case on the host (a mean near zero where the default's 4/64 over this many taps would make every neuron fire every step)
# so that the reference fires between 5 % and 95 % of the time in every run (tests/test_layer_major_cases.py).
# Byte stores (OH * OW no multiple of 4) with several blocks: stack_bytes, stack_analog and byte2_traces (81 and 63 pixels).
STACK = [("conv", 20, 3, 1, 1), ("conv", 16, 3, 1, 1), ("pool",), ("fc", 12), ("fc", 5)]
ZERO_MEAN = (-8, 8)
STACK_NUM = [(-4, 12), (-6, 8), None, (-7, 8), (-48, 64)]
STACK_NUM_ANALOG = [(-4, 10), (-6, 8), None, (-7, 8), (-48, 64)]
CASES = {
    "c3_5_5x5": (((3, 5, 5), [("conv", 5, 3, 1, 1)]), 7, 3, {}, None),
    "c17_16_9x7_refrac": (((17, 9, 7), [("conv", 16, 3, 1, 1)]), 7, 1, dict(refrac=2), None),
    "c32_20_9x7_lbound": (((32, 9, 7), [("conv", 20, 3, 1, 1)]), 2, 3, dict(lbound=-0.25), None),
    "stride2": (((17, 9, 7), [("conv", 20, 3, 2, 1)]), 7, 3, dict(refrac=2), None),
    "k1_T1": (((32, 5, 5), [("conv", 5, 1, 1, 0)]), 1, 1, {}, None),
    # a 5x5 bank of 97 -> 5 channels pads to 25 * 112 = 2800 terms = 44 slabs x 4 KiB = 176 KiB per channel group, beyond the 150 KiB the
    # kernel may ask for: the weights stream through two slabs every step
    "stream": (((97, 5, 5), [("conv", 5, 5, 1, 2)]), 2, 1, dict(density=0.1), lambda g: not g["resident"] and g["slabs"] == 44),
    "byte2_traces": (((17, 9, 7), [("conv", 20, 3, 1, 1), ("conv", 5, 3, 1, 1)]), 7, 3, dict(two=[(0, 2)], traces=True, trace_decay=0.5), None),
    "stack_bytes": (((3, 9, 9), STACK), 7, 3, {}, lambda g: not g["packed"] and g["blocks"] > 1),
    "stack_analog": (((3, 9, 9), STACK), 7, 3, dict(analog=True), None),
    # the same stacks, and the chain with traces, with numerators under which EVERY layer fires between 5 % and 95 % of the time in
    # both runs (the three above saturate in the second run from the second layer on, where an equal train or trace then says
    # little): for the time chunks of route 2, whose widest layers the stacks' are, and for the trace x against the reference
    "byte2_traces_sparse": (((17, 9, 7), [("conv", 20, 3, 1, 1), ("conv", 5, 3, 1, 1)]), 7, 3,
                            dict(two=[(0, 2)], traces=True, trace_decay=0.5, num=[(-7, 8), (-6, 8)]), None),
    "stack_bytes_sparse": (((3, 9, 9), STACK), 7, 3, dict(num=STACK_NUM), None),
    "stack_analog_sparse": (((3, 9, 9), STACK), 7, 3, dict(analog=True, num=STACK_NUM_ANALOG), None),
    # the middle block reads 6 rows x 24 pixels x 20 words = 2880 band words, beyond the 2048 a workgroup holds in registers: the loop
    # behind the chains stages the rest; packed stores in three blocks
    "stage_overflow": (((64, 8, 24), [("conv", 5, 3, 1, 1)]), 4, 2, dict(num=ZERO_MEAN),
                       lambda g: max(g["words"]) == 2880 > STAGE_WORDS and g["resident"] and g["packed"] and g["blocks"] == 3),
    # 49 slabs: every other step starts on slab buffer 1
    "stream_odd": (((49, 7, 7), [("conv", 5, 7, 1, 3)]), 5, 1, dict(num=ZERO_MEAN), lambda g: not g["resident"] and g["slabs"] == 49),
    # ... with a scalar step (which walks no slab) between matrix steps: the frame that feeds step 2 of the first run, and the first
    # frame of the second run, which feeds its step 1
    "stream_odd_byte2": (((49, 7, 7), [("conv", 5, 7, 1, 3)]), 5, 1, dict(num=ZERO_MEAN, two=[(0, 1)]),
                         lambda g: not g["resident"] and g["slabs"] % 2 == 1),
    "stream_odd_byte2_run2": (((49, 7, 7), [("conv", 5, 7, 1, 3)]), 5, 1, dict(num=ZERO_MEAN, two=[(1, 0)]),
                              lambda g: not g["resident"] and g["slabs"] % 2 == 1),
    # the prefetch of "the next step's slab 0" consumed four times
    "stream_even_long": (((97, 5, 5), [("conv", 5, 5, 1, 2)]), 5, 1, dict(density=0.1, num=ZERO_MEAN),
                         lambda g: not g["resident"] and g["slabs"] % 2 == 0),
    # 80 pixels: packed stores, block 1 with one live tile and three dead ones; two channel groups, 4 live channels in the second
    "packed_dead_tiles": (((17, 8, 10), [("conv", 20, 3, 1, 1)]), 4, 3, dict(num=(-7, 8)),
                          lambda g: g["packed"] and g["blocks"] == 2 and g["last_live_tiles"] == 1 and g["groups"] == 2 and g["last_group_channels"] == 4),
    "kh5_kw3": (((17, 9, 7), [("conv", 5, (5, 3), 1, 1)]), 4, 2, dict(num=(-7, 8)), lambda g: (g["KH"], g["KW"], g["OH"], g["OW"]) == (5, 3, 7, 7)),
    "kh5_kw3_stride2": (((17, 9, 7), [("conv", 5, (5, 3), 2, 1)]), 4, 2, dict(num=(-7, 8)), lambda g: (g["KH"], g["KW"], g["OH"], g["OW"]) == (5, 3, 4, 4)),
    "kh1_kw3": (((17, 9, 7), [("conv", 5, (1, 3), 1, 1)]), 4, 2, dict(density=0.5, num=(-6, 8)), lambda g: (g["KH"], g["KW"], g["OH"], g["OW"]) == (1, 3, 11, 7)),
    "kh1_kw3_stride2": (((17, 9, 7), [("conv", 5, (1, 3), 2, 1)]), 4, 2, dict(density=0.5, num=(-6, 8)), lambda g: (g["KH"], g["KW"], g["OH"], g["OW"]) == (1, 3, 6, 4)),
    # pad 2 under a 3x3: OH > H, the border windows hold one input pixel
    "pad_beyond_half": (((17, 5, 5), [("conv", 5, 3, 1, 2)]), 4, 2, dict(num=(-6, 8)), lambda g: g["pad"] > g["KH"] // 2 and g["OH"] == 7 > g["H"]),
    "pad0_cout1": (((17, 5, 5), [("conv", 1, 3, 1, 0)]), 4, 2, dict(num=(-6, 8)), lambda g: g["pad"] == 0 and g["Cout"] == 1 and g["nps"] == 9),
    # a convolution over spike bytes that the kernel refuses (two band buffers of 4 x 1200 pixels x 16 bytes = 150 KiB leave no room for
    # the slabs): route 2 propagates it
    "refused_bytes": (((3, 4, 1200), [("conv", 2, 3, 1, 1)]), 7, 3, {}, None),
}
# the cases whose reference must fire between 5 % and 95 % of the time in every run (everything this table gained after its first nine)
NEW = [name for name in CASES if name not in ("c3_5_5x5", "c17_16_9x7_refrac", "c32_20_9x7_lbound", "stride2", "k1_T1", "stream", "byte2_traces",
                                              "stack_bytes", "stack_analog")]


def inputs_of(name):
    spec, T, B, opt, _ = CASES[name]
    xs = [spike_input(spec, T, B, seed, opt.get("density", 0.3), opt.get("analog", False)) for seed in (11, 12)]
    for run, frame in opt.get("two", ()):
        xs[run][min(frame, T - 1), B - 1, 1, 2, 3] = 2             # one byte above 1: that workgroup's next step takes the scalar body
    return xs


def options(opt):
    return dict(refrac=opt.get("refrac", 0), lbound=opt.get("lbound"), traces=opt.get("traces", False), trace_decay=opt.get("trace_decay"))


_references = {}


def references(name):
    """(weights on the grid, inputs, [per run: (trains, state behind the run)]) of a case: computed once, shared, never written to."""
    if name not in _references:
        spec, T, B, opt, _ = CASES[name]
        ws, xs, state, runs = weights(spec, 5, grid=True, num=opt.get("num", (-4, 12))), inputs_of(name), {}, []
        for x in xs:
            traces = (opt["trace_decay"], 1.0, False) if opt.get("traces") else None      # (the layers' default scale, set not added)
            trains = reference(spec, ws, x, state, opt.get("refrac", 0), opt.get("lbound"), traces)
            runs.append((trains, {k: (v.clone() if isinstance(v, torch.Tensor) else [t.clone() for t in v]) for k, v in state.items()}))
        _references[name] = (ws, xs, runs)
    return _references[name]


# ... and whose every layer must
EVERY_LAYER = ("byte2_traces_sparse", "stack_bytes_sparse", "stack_analog_sparse")


def spike_share(trains):
    """The share of ones in the output train (the last layer's)."""
    return float(trains[-1].double().mean())


def byte2_frames(name):
    """[(run, frame)] of the case's input frames that hold a byte above 1 (all other bytes are 0 or 1; a frame holds no byte above 2)."""
    xs = inputs_of(name)
    assert all(int(x.max()) <= 2 for x in xs)
    return [(r, t) for r, x in enumerate(xs) for t in range(x.shape[0]) if int(x[t].max()) == 2]
