"""What the tests of snn_run_dense_sif_f32 share: the shapes, and a case's operands with their plain float64 reference (the one-layer "fc"
chain of tests/layer_major_cases.py over 2 T steps, from a non-zero entry state).  Weights, bias and state are on the 1/64 grid, numerators
at most 48 over at most 460 sources and bytes of at most 2, 140 steps at the most: every sum stays far below 2^24 / 64 and is exact in
float32 in any order, so the float64 result is the only correct one.  Trace decay 0.5, scale 1, set not added: x is a 1/64 value times a
power of two."""
import numpy as np
import torch

from layer_major_cases import reference, spike_input, weights

# name: (T, B, Nin, N), each the smallest at which something else can go wrong
SHAPES = {
    "one": (1, 1, 1, 1),                  # s_train is None
    "t16": (16, 1, 4, 16),                # one full time block, one full column tile
    "tails": (17, 2, 5, 17),              # a second time block, a K tail, a column tail in a second wave
    "blocks": (35, 3, 67, 33),            # three time blocks: the state crosses lane groups and blocks; a second slab with a tail
    "k300": (7, 3, 300, 20),              # five slabs, resident
    "super2": (70, 1, 70, 5),             # a second super block over a resident panel
    "streaming": (66, 2, 460, 70),        # eight slabs streaming twice, two panels, the second with 6 live columns
}
TRACES = (0.5, 1.0, False)


def entry_state(shape, seed, refrac):
    rng = np.random.default_rng(seed)
    rc = rng.integers(0, refrac + 1, shape) * (rng.random(shape) < 0.5) if refrac else np.zeros(shape)
    return {k: torch.from_numpy(np.asarray(a, np.float64)) for k, a in
            dict(v=rng.integers(-32, 64, shape) / 64.0, rc=rc, summed=rng.integers(-64, 65, shape) / 64.0, x=rng.integers(0, 65, shape) / 64.0).items()}


def case(name, bias, refrac, traces, two=False, grid=True):
    """(W [Nin, N], b or None, s0 [B, Nin], x [2T, B, Nin], entry state, reference train [2T, B, N], reference state behind it)."""
    T, B, Nin, N = SHAPES[name]
    spec = ((Nin,), [("fc", N)])
    (W, b), = weights(spec, 5, grid=grid, num=(-8, 8) if Nin > 16 else (-16, 48))
    x, s0 = spike_input(spec, 2 * T, B, 31), spike_input(spec, 1, B, 32)[0]
    if two:                                # read by step T + 1, by step T where T == 1: the first super block of a second call of T, sample B - 1
        x[T - 1 + (T > 1), B - 1, Nin // 2] = 2
    ent, state = entry_state((B, N), 33, refrac), {}
    want = reference(spec, [(W, b if bias else torch.zeros_like(b))], x, state, refrac, None, TRACES if traces else None,
                     entry=dict(s=[s0, torch.zeros(B, N)], v=[ent["v"]], rc=[ent["rc"]], x=[ent["x"]], summed=ent["summed"]))[0]
    return W, (b if bias else None), s0, x, ent, want, state
