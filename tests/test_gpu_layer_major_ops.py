"""The two operators of the layer-major plan called directly: ops.run_conv2d_sif (snn_run_conv2d_sif_f32) and ops.sif_scan (snn_sif_scan)
against the plain float64 reference of tests/layer_major_cases.py, exactly (weights, currents and state on a 1/64 grid, trace decay 0.5
and scale 1), from a NON-zero entry state -- v, refrac_count with neurons mid-refractory, summed, x, and a non-zero start frame --, with
every output tensor inside a guard of sentinel bytes that must come back untouched."""
import numpy as np
import pytest
import torch

from layer_major_cases import CASES, geometry, if_step, reference, shapes, spike_input, trace_next, weights

pytestmark = pytest.mark.gpu
GUARD = 256                                                         # bytes on either side


def guarded(t, shift=0):
    """`t` on the device as a contiguous view inside a larger buffer: (view, buffer, the buffer as it was).  `shift`: extra bytes in
    front, so that a byte tensor starts at an address that is no multiple of 4."""
    lead = (GUARD + shift) // t.element_size()
    fill = 0xA5 if t.dtype == torch.uint8 else -777.25
    buf = torch.full((lead + t.numel() + GUARD // t.element_size(),), fill, dtype=t.dtype, device="cuda")
    view = buf[lead:lead + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf, buf.clone()


def assert_guards_untouched(cells):
    for name, (view, buf, before) in cells.items():
        lead = view.data_ptr() - buf.data_ptr()
        lead //= buf.element_size()
        assert torch.equal(buf[:lead], before[:lead]) and torch.equal(buf[lead + view.numel():], before[lead + view.numel():]), f"guard of {name}"


def lif(refrac=0, lbound=None, traces=None):
    from bindsnet_amd._lib import LifParams
    decay, scale, additive = traces or (0.0, 1.0, False)
    return LifParams(decay=1.0, rest=0.0, reset=0.0, thresh=1.0, refrac=float(refrac), dt=1.0, has_lbound=int(lbound is not None),
                     lbound=float(lbound or 0.0), traces=int(traces is not None), trace_decay=decay, trace_scale=scale, traces_additive=int(additive))


def entry_state(shape, seed, refrac):
    """v, refrac_count, summed, x [*shape] on the 1/64 grid; a third of the neurons mid-refractory where the layer has a refractory period."""
    rng = np.random.default_rng(seed)
    rc = rng.integers(0, refrac + 1, shape) * (rng.random(shape) < 0.5) if refrac else np.zeros(shape)
    return {k: torch.from_numpy(np.asarray(a, np.float64)) for k, a in
            dict(v=rng.integers(-32, 64, shape) / 64.0, rc=rc, summed=rng.integers(-64, 65, shape) / 64.0, x=rng.integers(0, 65, shape) / 64.0).items()}


# name: (the case of layer_major_cases whose shape and numerators it takes, T (None: the case's), refrac, lbound, traces (decay, scale,
# additive), with summed, shift of the byte tensors)
CONV = {
    "resident": ("packed_dead_tiles", None, 2, None, (0.5, 1.0, False), True, 0),
    "streaming": ("stream_odd", None, 0, None, (0.5, 1.0, True), True, 0),
    "non_square": ("kh5_kw3_stride2", None, 2, None, (0.5, 1.0, False), True, 0),
    "overflow": ("stage_overflow", None, 0, None, None, True, 0),
    "no_summed": ("packed_dead_tiles", None, 2, None, (0.5, 1.0, False), False, 0),
    "no_traces": ("packed_dead_tiles", None, 2, None, None, True, 0),
    "additive": ("packed_dead_tiles", None, 2, None, (0.5, 1.0, True), True, 0),
    "T1": ("packed_dead_tiles", 1, 2, None, (0.5, 1.0, False), True, 0),
    "lbound": ("packed_dead_tiles", None, 0, -0.25, (0.5, 1.0, False), True, 0),
    # a pixel count that is a multiple of 4 behind an address that is not: the byte stores of the packed shapes (ops._ptr takes the view)
    "unaligned": ("packed_dead_tiles", None, 2, None, (0.5, 1.0, False), True, 1),
    "unaligned_overflow": ("stage_overflow", None, 0, None, None, True, 3),
}


def conv_case(name):
    """(spec, weights, start frame, input, entry state, reference trains and state) on the host."""
    case, T, refrac, lbound, traces, sums, shift = CONV[name]
    spec, T0, B, opt, _ = CASES[case]
    T = T or T0
    ws = weights(spec, 5, grid=True, num=opt.get("num", (-4, 12)))
    x, s0 = spike_input(spec, T, B, 31, opt.get("density", 0.3)), spike_input(spec, 1, B, 32, opt.get("density", 0.3))[0]
    ent = entry_state((B, *shapes(spec)[0]), 33, refrac)
    state = {}
    want = reference(spec, ws, x, state, refrac, lbound, traces,
                     entry=dict(s=[s0, torch.zeros(B, *shapes(spec)[0])], v=[ent["v"]], rc=[ent["rc"]], x=[ent["x"]], summed=ent["summed"]))[0]
    return spec, ws, s0, x, ent, want, state


@pytest.mark.parametrize("name", list(CONV))
def test_run_conv2d_sif_equals_the_float64_reference(name):
    from bindsnet_amd import ops
    case, T, refrac, lbound, traces, sums, shift = CONV[name]
    spec, ws, s0, x, ent, want, state = conv_case(name)
    T, B = x.shape[:2]
    op, g = spec[1][0], geometry(spec)
    assert 0.05 <= float(want.double().mean()) <= 0.95 and (shift == 0 or g["packed"])
    if refrac:
        assert 0.1 < float((ent["rc"] > 0).double().mean()) < 0.6
    assert ops.run_conv2d_sif_takes(T, B, *spec[0], op[1], g["KH"], g["KW"], op[3], op[4]) == (1 if g["resident"] else 2)

    cells = dict(train=guarded(torch.full(want.shape, 9, dtype=torch.uint8), shift), s=guarded(torch.full(want.shape[1:], 9, dtype=torch.uint8), shift),
                 v=guarded(ent["v"].float()), rc=guarded(ent["rc"].float()))
    if sums:
        cells["summed"] = guarded(ent["summed"].float())
    if traces:
        cells["x"] = guarded(ent["x"].float())
    assert shift == 0 or cells["train"][0].data_ptr() % 4 != 0
    view = lambda k: cells[k][0] if k in cells else None           # noqa: E731
    # (frames 0 .. T-2 of the source's train are read and no more: only those are passed)
    ops.run_conv2d_sif(ws[0][0].cuda(), ws[0][1].cuda(), s0.cuda(), x[:T - 1].cuda() if T > 1 else None, view("train"), view("v"), view("rc"),
                       view("s"), lif(refrac, lbound, traces), x=view("x"), summed=view("summed"), stride=op[3], pad=op[4])
    torch.cuda.synchronize()
    assert torch.equal(view("train").cpu(), want), "train"
    assert torch.equal(view("s").cpu(), want[-1]), "s"
    assert torch.equal(view("v").cpu().double(), state["v"][0]), "v"
    assert torch.equal(view("rc").cpu().double(), state["rc"][0]), "refrac_count"
    if sums:
        assert torch.equal(view("summed").cpu().double(), state["summed"]), "summed"
    if traces:
        assert torch.equal(view("x").cpu().double(), state["x"][0]), "x"
    assert_guards_untouched(cells)


SPLITS = ((7,), (1, 6), (3, 4), (1,) * 7)


@pytest.mark.parametrize("N", (1, 255, 256, 257))
def test_sif_scan_in_any_chunks_equals_the_float64_reference(N):
    """T = 7 steps of B x N neurons in one call and in chunks of 1 + 6, 3 + 4 and 7 x 1, with and without `summed`, with and without
    traces: the same train and state every time.  (N around the workgroup's 256 threads: the last workgroup is partial.)"""
    from bindsnet_amd import ops
    T, B, refrac, traces_on = 7, 3, 2, (0.5, 1.0, True)
    rng = np.random.default_rng(40 + N)
    I = torch.from_numpy(rng.integers(-32, 65, (T, B, N)) / 64.0)
    ent = entry_state((B, N), 41, refrac)
    for sums in (True, False):
        for traces in (traces_on, None):
            v, rc, summed, x = (ent[k].clone() for k in ("v", "rc", "summed", "x"))
            want = torch.zeros(T, B, N, dtype=torch.uint8)
            for t in range(T):
                s = if_step(v, rc, I[t], refrac)
                if traces:
                    x = trace_next(x, s.double(), *traces)
                summed += I[t]
                want[t] = s
            assert 0.05 <= float(want.double().mean()) <= 0.95
            for split in SPLITS:
                cells = dict(train=guarded(torch.full((T, B, N), 9, dtype=torch.uint8)), s=guarded(torch.full((B, N), 9, dtype=torch.uint8)),
                             v=guarded(ent["v"].float()), rc=guarded(ent["rc"].float()))
                if sums:
                    cells["summed"] = guarded(ent["summed"].float())
                if traces:
                    cells["x"] = guarded(ent["x"].float())
                view = lambda k: cells[k][0] if k in cells else None           # noqa: E731
                cur, t0 = I.float().cuda(), 0
                for Tc in split:
                    ops.sif_scan(view("v"), view("rc"), view("s"), view("x"), cur[t0:t0 + Tc], view("train")[t0:t0 + Tc], lif(refrac, None, traces),
                                 summed=view("summed"))
                    t0 += Tc
                torch.cuda.synchronize()
                what = f"split {split}, summed {sums}, traces {traces is not None}"
                assert torch.equal(view("train").cpu(), want) and torch.equal(view("s").cpu(), want[-1]), what
                assert torch.equal(view("v").cpu().double(), v) and torch.equal(view("rc").cpu().double(), rc), what
                assert not sums or torch.equal(view("summed").cpu().double(), summed), what
                assert not traces or torch.equal(view("x").cpu().double(), x), what
                assert_guards_untouched(cells)
