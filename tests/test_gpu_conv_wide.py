"""Conv2dConnection with more than 16 input channels, or a filter bank beyond 64 KiB, on the device (csrc/snn_conv_wide.hip).

Kernel sweep: ops.prop_conv2d against oracle.prop_conv2d (the stated order: sequential f32 over (kh, kw, cin), bias last) bit for bit,
real-valued weights and bias, with and without accumulate, densities 0, 0.01, 0.3 and 1.  The product Cin {17, 32, 64, 100} x
Cout {1, 8, 9, 40, 130} x kernel {1x1, 3x3, 5x3} x (stride, pad) {(1, 0), (1, 1), (2, 2)} x image {6x7, 1x1} x B {1, 3} is thinned to
every fifth combination (each value of each factor stays, asserted); KEPT is run whole.  The per-workgroup limits of the kernel and
the kept shapes on either side of them:
  * 8 output channels per workgroup: Cout 1 (one lane of the chunk), 8 (one full chunk), 9 (a full chunk and one channel), 40, 130, 300;
  * slabs of 512 ordered taps: Cin 17 x 3x3 = 153 (one slab); Cin 64 x 3x3 = 576 (two, cut exactly between two tap positions);
    Cin 100 x 5x3 = 1500 (three, both cuts inside a tap position's channels and inside a group of 16 channels); Cin 8 x 3x3 = 72;
  * groups of 16 input channels per LDS read: Cin 17 (one group and one channel), 100 (six groups and four), 8 (half a group), 32, 64;
  * 256 output pixels per workgroup: 6x7 at B 3 = 126 (one partial block), 1x1 at B 3 (3 pixels, every pixel another sample, more
    samples per block allowed than the batch has), 20x19 at B 3 = 1140 (five blocks, blocks that span two samples);
  * 48 KiB of staged images per workgroup: Cin 17 on 33x32 at B 2 needs 99 KiB, so the spikes are read from global memory;
  * the old kernel's limits: Cin 64 x Cout 40 x 3x3 is a 92 KiB bank with Cin > 16; Cin 8 x Cout 300 x 3x3 is 86 KiB with Cin <= 16,
    refused before for the bank alone; Cin 16 x Cout 8 x 3x3 still takes the old kernel and must equal the same oracle.

Then every fixture case of tests/conv_wide_cases.py on the device against the reference fixture bit for bit on the generic plan, two
half runs against one, the device against F.conv2d on the CPU for real-valued weights within the derived summation bound, and the
refusals."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_wide_cases as WC
import oracle
from test_conv_wide_host import _bits, _conv, _ns, built, check_snapshots

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32

CINS, COUTS = (17, 32, 64, 100), (1, 8, 9, 40, 130)
KERNELS, GEOMS, IMAGES, BATCHES = ((1, 1), (3, 3), (5, 3)), ((1, 0), (1, 1), (2, 2)), ((6, 7), (1, 1)), (1, 3)
DENSITIES = (0.0, 0.01, 0.3, 1.0)
# (Cin, Cout, (KH, KW), (stride, pad), (H, W), B)
KEPT = [
    (17, 9, (3, 3), (1, 1), (6, 7), 3), (17, 1, (5, 3), (2, 2), (6, 7), 1), (64, 40, (3, 3), (1, 1), (6, 7), 3),
    (8, 300, (3, 3), (1, 1), (6, 7), 3), (100, 9, (5, 3), (1, 1), (6, 7), 3), (100, 1, (3, 3), (1, 1), (1, 1), 3),
    (32, 9, (1, 1), (1, 0), (1, 1), 1), (20, 9, (3, 3), (1, 1), (20, 19), 3), (17, 2, (3, 3), (1, 1), (33, 32), 2),
    (16, 8, (3, 3), (1, 1), (6, 7), 3),
]


def _valid(shape):
    cin, cout, (kh, kw), (stride, pad), (h, w), B = shape
    return h + 2 * pad >= kh and w + 2 * pad >= kw


def thinned():
    product = [s for s in itertools.product(CINS, COUTS, KERNELS, GEOMS, IMAGES, BATCHES) if _valid(s)]
    kept = product[::5]
    for axis, values in enumerate((CINS, COUTS, KERNELS, GEOMS, IMAGES, BATCHES)):
        assert {s[axis] for s in kept} == set(values), axis
    return kept


def check_shape(shape):
    from bindsnet_amd import ops
    cin, cout, (kh, kw), (stride, pad), (h, w), B = shape
    rng = np.random.default_rng(hash(shape) % (1 << 31))
    W, bias = rng.standard_normal((cout, cin, kh, kw)).astype(f32), rng.standard_normal(cout).astype(f32)
    Wd, bd = torch.from_numpy(W).to(DEV), torch.from_numpy(bias).to(DEV)
    for density in DENSITIES:
        s = (rng.random((B, cin, h, w)) < density).astype(np.uint8)
        want = oracle.prop_conv2d(W, s, bias=bias, stride=stride, pad=pad)
        prev = rng.standard_normal(want.shape).astype(f32)
        sd = torch.from_numpy(s).to(DEV)
        out = torch.full(want.shape, float("nan"), device=DEV)
        ops.prop_conv2d(Wd, sd, out, bias=bd, stride=stride, pad=pad)
        acc = torch.from_numpy(prev).to(DEV)
        ops.prop_conv2d(Wd, sd, acc, bias=None, stride=stride, pad=pad, accumulate=True)
        got, got_acc = out.cpu().numpy(), acc.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (shape, density, int((_bits(got) != _bits(want)).sum()))
        assert np.array_equal(_bits(got_acc), _bits(prev + oracle.prop_conv2d(W, s, stride=stride, pad=pad))), (shape, density, "accumulate")


@pytest.mark.parametrize("cin", CINS)
def test_sweep_equals_the_stated_order(cin):
    shapes = [s for s in thinned() if s[0] == cin]
    assert len(shapes) >= 20
    for shape in shapes:
        check_shape(shape)


@pytest.mark.parametrize("shape", KEPT, ids=lambda s: f"cin{s[0]}_cout{s[1]}_k{s[2][0]}x{s[2][1]}_s{s[3][0]}p{s[3][1]}_{s[4][0]}x{s[4][1]}_b{s[5]}")
def test_kept_shapes_equal_the_stated_order(shape):
    check_shape(shape)


@pytest.mark.parametrize("name", WC.NAMES)
def test_device_reproduces_fixture(name):
    g, net = built(name)
    net.to(DEV)
    snaps = WC.run_case(_ns(), net, name, device=DEV)
    assert net.last_plan == "generic"
    check_snapshots(name, snaps, g)


def test_two_halves_equal_one_whole_run_on_the_device():
    g, net = built("a")
    net.to(DEV)
    check_snapshots("a", WC.run_case(_ns(), net, "a", device=DEV, halves=True, count=1), g)
    assert net.last_plan == "generic"


def test_real_weights_against_the_reference_within_the_summation_bound():
    """Device (stated order) against F.conv2d on the CPU (oneDNN's order): both sum the same terms t_i -- the weights of the active
    taps, and the bias --, each sum of m terms is within gamma_m * sum |t_i| of the exact one (gamma_m = m u / (1 - m u), u = 2^-24), so
    the two differ by at most twice that.  Derived, not measured."""
    from bindsnet_amd import ops
    rng = np.random.default_rng(11)
    W, bias = rng.standard_normal((20, 100, 5, 5)).astype(f32), rng.standard_normal(20).astype(f32)
    s = (rng.random((2, 100, 9, 9)) < 0.3).astype(np.uint8)
    st = torch.from_numpy(s)
    ref = F.conv2d(st.float(), torch.from_numpy(W), torch.from_numpy(bias), padding=2).numpy()
    out = torch.empty(ref.shape, device=DEV)
    ops.prop_conv2d(torch.from_numpy(W).to(DEV), st.to(DEV), out, bias=torch.from_numpy(bias).to(DEV), stride=1, pad=2)
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(oracle.prop_conv2d(W, s, bias=bias, stride=1, pad=2)))
    s64 = st.double()
    m = F.conv2d(s64, torch.ones(1, 100, 5, 5, dtype=torch.float64), padding=2).numpy() + 1.0                       # active taps + the bias
    mag = F.conv2d(s64, torch.from_numpy(W).double().abs(), torch.from_numpy(bias).double().abs(), padding=2).numpy()
    u = 2.0 ** -24
    bound = 2.0 * (m * u / (1.0 - m * u)) * mag
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print(f"max |device - reference| {err.max():.3g}, least bound {bound.min():.3g}, largest err / bound {np.max(err / bound):.3g}, "
          f"{int((_bits(got) != _bits(ref)).sum())} of {got.size} elements differ")
    assert (err <= bound).all(), float(np.max(err / bound))


def test_refusals_on_the_device():
    from bindsnet_amd import learning
    ns = _ns()
    for rule in ("PostPre", "Hebbian", "WeightDependentPostPre", "MSTDP"):
        with pytest.raises(NotImplementedError, match=f"{rule} on a Conv2dConnection with 17 input channels"):
            _conv(17, getattr(learning, rule), wmin=0.0, wmax=1.0)
    net = ns.Network(dt=1.0, batch_size=2)                 # NoOp at 17 channels runs, on the generic plan, and leaves the weights alone
    X, Y = ns.Input(shape=(17, 5, 5), traces=True), ns.LIFNodes(shape=(4, 3, 3), traces=True)
    rng = np.random.default_rng(5)
    conn = ns.Conv2dConnection(X, Y, kernel_size=3, update_rule=learning.NoOp, w=WC.grid(rng, 0, 64, 4, 17, 3, 3))
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(conn, "X", "Y")
    net.to(DEV)
    before = conn.w.detach().cpu().numpy().copy()
    mon = ns.Monitor(Y, ["s"], time=20)
    net.add_monitor(mon, "Y_s")
    net.run({"X": torch.from_numpy((rng.random((20, 2, 17, 5, 5)) < 0.3).astype(np.uint8)).to(DEV)}, time=20)
    assert net.last_plan == "generic" and int(mon.get("s").sum()) > 0
    assert np.array_equal(conn.w.detach().cpu().numpy(), before)
