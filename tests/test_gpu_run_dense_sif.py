"""snn_run_dense_sif_f32 on the device (ops.run_dense_sif; route 3 of network/layer_major.py): a Connection and its IF neurons over the
whole run in one launch, against the plain float64 reference (tests/run_dense_sif_cases.py: grid weights, equality is exact), bit for
bit against T x (ops.prop_dense + ops.sif_step) with randn weights and a byte 2, and through Network.run against the generic plan."""
import pytest
import torch

from layer_major_cases import build, spike_input, weights
from run_dense_sif_cases import SHAPES, TRACES, case
from test_gpu_layer_major import assert_same_bits, run_twice
from test_gpu_layer_major_ops import lif

pytestmark = pytest.mark.gpu
OPTIONS = {"plain": (True, 0, False, True), "bare": (False, 2, True, False)}       # bias, refrac, traces, summed


def fused(W, b, s0, x, ent, T, refrac, traces, sums):
    """Two calls of T steps on one state: (train [2T, B, N], state)."""
    from bindsnet_amd import ops
    B, N = ent["v"].shape
    st = {k: ent[k].float().cuda() for k in ("v", "rc", "summed", "x")}
    st["s"], train = torch.full((B, N), 9, dtype=torch.uint8, device="cuda"), torch.full((2 * T, B, N), 9, dtype=torch.uint8, device="cuda")
    Wd, bd, xd = W.cuda(), None if b is None else b.cuda(), x.cuda()
    for run, start in enumerate((s0.cuda(), xd[T - 1])):
        ops.run_dense_sif(Wd, bd, start, xd[run * T:(run + 1) * T - 1] if T > 1 else None, train[run * T:(run + 1) * T], st["v"], st["rc"], st["s"],
                          lif(refrac, None, TRACES if traces else None), x=st["x"] if traces else None, summed=st["summed"] if sums else None)
    return train.cpu(), {k: t.cpu() for k, t in st.items()}


@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_equals_the_float64_reference(name, opt):
    from bindsnet_amd import ops
    bias, refrac, traces, sums = OPTIONS[opt]
    T, B, Nin, N = SHAPES[name]
    assert ops.run_dense_sif_takes(T, B, Nin, N) == (2 if name == "streaming" else 1)
    W, b, s0, x, ent, want, state = case(name, bias, refrac, traces)
    train, st = fused(W, b, s0, x, ent, T, refrac, traces, sums)
    assert torch.equal(train, want) and torch.equal(st["s"], want[-1])
    for key in ("v", "rc") + (("summed",) if sums else ()) + (("x",) if traces else ()):
        assert torch.equal(st[key].double(), state[key] if key == "summed" else state[key][0]), key


@pytest.mark.parametrize("two", (False, True), ids=("bytes01", "byte2"))
@pytest.mark.parametrize("name", list(SHAPES))
def test_equals_the_generic_steps_bit_for_bit(name, two):
    """randn weights: the order must be the event-driven kernel's, with a byte 2 in a frame too."""
    from bindsnet_amd import ops
    T, B, Nin, N = SHAPES[name]
    W, b, s0, x, ent, _, _ = case(name, True, 2, True, two, grid=False)
    train, st = fused(W, b, s0, x, ent, T, 2, True, True)
    g = {k: ent[k].float().cuda() for k in ("v", "rc", "summed", "x")}
    s, I, Wd, bd = torch.zeros(B, N, dtype=torch.uint8, device="cuda"), torch.empty(B, N, device="cuda"), W.cuda(), b.cuda()
    frames = torch.cat((s0[None], x[:2 * T - 1])).cuda()
    for t in range(2 * T):
        ops.prop_dense(Wd, frames[t], I, bias=bd)
        ops.sif_step(g["v"], g["rc"], s, g["x"], I, lif(2, None, TRACES), summed=g["summed"])
        assert torch.equal(train[t], s.cpu()), f"train of step {t}"
    for key in g:
        assert torch.equal(st[key].view(torch.int32), g[key].cpu().view(torch.int32)), key


def test_a_dense_chain_runs_one_launch_per_layer(monkeypatch):
    from bindsnet_amd import ops
    spec, T, B = ((20,), [("fc", 33), ("fc", 17), ("fc", 5)]), 20, 3
    ws, xs = weights(spec, 6, grid=False), [spike_input(spec, T, B, seed) for seed in (11, 12)]
    calls = {"run_dense_sif": 0, "sif_scan": 0}
    for fn in calls:
        def spy(*a, _fn=fn, _real=getattr(ops, fn), **kw):
            calls[_fn] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, fn, spy)
    runs = run_twice(build(spec, ws, B, True, refrac=2, traces=True).to("cuda"), xs)
    assert calls == {"run_dense_sif": 6, "sif_scan": 0}                            # three layers, two runs
    generic = run_twice(build(spec, ws, B, False, refrac=2, traces=True).to("cuda"), xs)
    assert all(0 < float(t.double().mean()) < 1 for t in generic[1][0])
    assert_same_bits(runs, generic)


def test_takes_answers_from_the_shape_alone():
    from bindsnet_amd import ops
    assert ops.run_dense_sif_takes(100, 16, 448, 10) == 1 and ops.run_dense_sif_takes(100, 16, 449, 10) == 2
    assert ops.run_dense_sif_takes(1, 65535, 1 << 10, 1) == 2 and ops.run_dense_sif_takes((1 << 31) - 1, 1, 1, 1) == 1
    for shape in ((0, 1, 1, 1), (1, 65536, 1, 1), (1, 1, 1 << 24, 1), (1 << 16, 1 << 15, 1, 1), (1 << 15, 1, 1, 1 << 16), (1 << 15, 1, 1 << 16, 1)):
        assert ops.run_dense_sif_takes(*shape) == 0, shape
