"""What the AvgPool2dConnection / fold_batchnorm tests share (tests/test_avgpool_host.py, test_avgpool_hostcheck.py,
test_gpu_avgpool.py): the 576 pooling geometries with their spikes and torch's own result (computed once), the small CNN with
BatchNorm and average pooling on a dyadic grid, the pooling graph of the device run, and a converted network's run written out
as a plain-torch step loop."""
import functools
import itertools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

PLANES = ((7, 5), (6, 6), (9, 11))
KERNELS = ((2, 2), (3, 3), (2, 3), (6, 5))
STRIDES = ((2, 2), (1, 2), (3, 3))
PADS = (0, 1)
B, C = 3, 4

# (plane, kernel, stride, pad, ceil_mode, count_include_pad): 3 * 4 * 3 * 2 * 2 * 2 = 288, each without a divisor_override and with 3: 576 cases
GEOMETRIES = tuple(itertools.product(PLANES, KERNELS, STRIDES, PADS, (False, True), (False, True)))
DIVISORS = (None, 3)


@functools.lru_cache(maxsize=None)
def spikes(plane, dtype=torch.uint8, b=B, c=C):
    """0/1 spikes [b, c, *plane] at a rate near one half, the same for every test that names the plane."""
    gen = torch.Generator().manual_seed(1000 * plane[0] + plane[1] + 17 * b + c)
    return (torch.rand(b, c, *plane, generator=gen) < 0.5).to(dtype)


def pool_kwargs(geometry, divisor=None):
    plane, k, stride, pad, ceil_mode, include = geometry
    return dict(kernel_size=k, stride=stride, padding=pad, ceil_mode=ceil_mode, count_include_pad=include, divisor_override=divisor)


@functools.lru_cache(maxsize=None)
def reference(geometry, divisor=None):
    """F.avg_pool2d on the CPU over spikes(plane): the oracle.  Never written to."""
    return F.avg_pool2d(spikes(geometry[0]).float(), **pool_kwargs(geometry, divisor))


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---- the model of tools/bench_avgpool.py scaled to a (2, 8, 8) input, every parameter on a dyadic grid ------------------------------

INPUT = (2, 8, 8)
MODEL_LAYERS = [("Input", "Input", [2, 8, 8]), ("1", "SubtractiveResetIFNodes", [4, 8, 8]), ("4", "SubtractiveResetIFNodes", [4, 4, 4]),
                ("5", "SubtractiveResetIFNodes", [6, 4, 4]), ("8", "SubtractiveResetIFNodes", [6, 1, 1]), ("10", "SubtractiveResetIFNodes", [5])]
MODEL_CONNECTIONS = [(["0", "1"], "Conv2dConnection"), (["3", "4"], "AvgPool2dConnection"), (["4", "5"], "Conv2dConnection"),
                     (["7", "8"], "AvgPool2dConnection"), (["9", "10"], "Connection")]


def _grid(gen, shape, denom, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float() / denom


def model(seed=5, dyadic=True):
    """Conv-BN-ReLU-AvgPool2-Conv-BN-ReLU-AdaptiveAvgPool(1)-Flatten-Linear in eval mode.  dyadic: weights on a 1/64 grid, BatchNorm with
    eps = 0, running_var in {1/4, 1, 4} and gamma in {1/2, 1, 2} -- every scale gamma / sqrt(var + eps) a power of two -- and means and
    betas on a 1/8 grid, so folding is exact and every partial sum of a run over 0/1 spikes is exact in float32 in any order."""
    gen = torch.Generator().manual_seed(seed)
    ann = nn.Sequential(nn.Conv2d(2, 4, 3, padding=1), nn.BatchNorm2d(4), nn.ReLU(), nn.AvgPool2d(2), nn.Conv2d(4, 6, 3, padding=1, bias=False),
                        nn.BatchNorm2d(6), nn.ReLU(), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(6, 5))
    with torch.no_grad():
        for m in ann:
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                m.weight.copy_(_grid(gen, m.weight.shape, 64, -12, 24) if dyadic else torch.randn(m.weight.shape, generator=gen) / 3)
                if m.bias is not None:
                    m.bias.copy_(_grid(gen, m.bias.shape, 64, -8, 8) if dyadic else torch.randn(m.bias.shape, generator=gen) / 8)
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                if dyadic:
                    m.eps = 0.0
                    m.running_var.copy_(torch.tensor([0.25, 1.0, 4.0])[torch.randint(0, 3, (n,), generator=gen)])
                    m.weight.copy_(torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=gen)])
                    m.running_mean.copy_(_grid(gen, (n,), 8, -2, 2))
                    m.bias.copy_(_grid(gen, (n,), 8, -1, 2))
                else:
                    m.running_var.copy_(torch.rand(n, generator=gen) + 0.5)
                    m.weight.copy_(torch.rand(n, generator=gen) + 0.5)
                    m.running_mean.copy_(torch.randn(n, generator=gen) / 4)
                    m.bias.copy_(torch.randn(n, generator=gen) / 4)
    return ann.eval()


def model_input(T, b, seed=9):
    gen = torch.Generator().manual_seed(seed + b)
    return (torch.rand(T, b, *INPUT, generator=gen) < 0.5).to(torch.uint8)


def step_loop(ann, x):
    """A converted `ann` (model() above, BatchNorm folded by hand here: y = conv(s) * scale + shift) over the spike train x [T, B, 2, 8, 8],
    as plain torch: every layer reads its source's spikes of the step before, then  v += current; s = v >= 1; v -= s.  Returns
    ({layer name: raster [T, B, ...]}, {layer name: v}, summed of the last layer)."""
    conv1, bn1, _, pool, conv2, bn2, _, _, _, lin = ann

    def folded(conv, bn):
        scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        bias = conv.bias.double() if conv.bias is not None else torch.zeros_like(scale)
        return (conv.weight.double() * scale.view(-1, 1, 1, 1)).float(), ((bias - bn.running_mean.double()) * scale + bn.bias.double()).float()

    (w1, b1), (w2, b2) = folded(conv1, bn1), folded(conv2, bn2)
    T, nb = x.shape[:2]
    feeds = {"1": lambda s: F.conv2d(s["Input"], w1, b1, padding=1), "4": lambda s: F.avg_pool2d(s["1"], pool.kernel_size),
             "5": lambda s: F.conv2d(s["4"], w2, b2, padding=1), "8": lambda s: F.avg_pool2d(s["5"], 4),
             "10": lambda s: F.linear(s["8"].flatten(1), lin.weight, lin.bias)}
    shapes = {name: shape for name, _, shape in MODEL_LAYERS}
    s = {name: torch.zeros(nb, *shape) for name, shape in shapes.items()}
    v = {name: torch.zeros(nb, *shapes[name]) for name in feeds}
    summed = torch.zeros(nb, 5)
    rasters = {name: [] for name in feeds}
    with torch.no_grad():
        for t in range(T):
            cur = {name: feed(s) for name, feed in feeds.items()}          # (all from the spikes of the step before)
            s["Input"] = x[t].float()
            for name in feeds:
                v[name] = v[name] + cur[name]
                fired = v[name] >= 1
                v[name] = v[name] - fired.float()
                s[name] = fired.float()
                rasters[name].append(fired)
            summed = summed + cur["10"]
    return {name: torch.stack(r) for name, r in rasters.items()}, v, summed


def run_converted(net, x, Monitor, halves=False):
    """One run of a converted network over x [T, B, ...] on whatever device it lives on: ({layer: raster}, {layer: v}, summed of the last)."""
    T = x.shape[0]
    names = [n for n in net.layers if n != "Input"]
    for n in names:
        net.add_monitor(Monitor(net.layers[n], ["s"], time=T), name=f"{n}_s")
    if halves:
        h = T // 2
        net.run({"Input": x[:h].clone()}, time=h)
        net.run({"Input": x[h:].clone()}, time=T - h)
    else:
        net.run({"Input": x}, time=T)
    rasters = {n: net.monitors[f"{n}_s"].get("s").cpu() != 0 for n in names}
    v = {n: net.layers[n].v.detach().cpu().clone() for n in names}
    return rasters, v, net.layers[names[-1]].summed.detach().cpu().clone()


def pool_graph(ns_nodes, topology, Network, b, seed=3):
    """Input(2, 8, 8) -> Conv2d(4, k 3, pad 1), weights on a 1/64 grid -> IF -> AvgPool2d(2) -> IF -> Connection -> IF(sum_input)."""
    gen = torch.Generator().manual_seed(seed)
    net = Network(dt=1.0, batch_size=b)
    X = ns_nodes["Input"](shape=INPUT)
    A = ns_nodes["SIF"](shape=(4, 8, 8), reset=0, thresh=1, refrac=0)
    P = ns_nodes["SIF"](shape=(4, 4, 4), reset=0, thresh=1, refrac=0)
    Y = ns_nodes["SIF"](n=5, reset=0, thresh=1, refrac=0, sum_input=True)
    for name, layer in (("X", X), ("A", A), ("P", P), ("Y", Y)):
        net.add_layer(layer, name=name)
    net.add_connection(topology.Conv2dConnection(X, A, kernel_size=3, padding=1, w=_grid(gen, (4, 2, 3, 3), 64, -8, 20),
                                                 b=_grid(gen, (4,), 64, -4, 4)), "X", "A")
    net.add_connection(topology.AvgPool2dConnection(A, P, kernel_size=2), "A", "P")
    net.add_connection(topology.Connection(P, Y, w=_grid(gen, (64, 5), 64, -8, 16), b=_grid(gen, (5,), 64, -4, 4)), "P", "Y")
    return net


def np_fold(w, b, gamma, beta, mean, var, eps):
    """fold_batchnorm's rule restated in numpy float64 (b None: zeros; gamma / beta None: ones / zeros), cast to float32 once."""
    w, mean, var = np.asarray(w, np.float64), np.asarray(mean, np.float64), np.asarray(var, np.float64)
    n = w.shape[0]
    gamma = np.ones(n) if gamma is None else np.asarray(gamma, np.float64)
    beta = np.zeros(n) if beta is None else np.asarray(beta, np.float64)
    b = np.zeros(n) if b is None else np.asarray(b, np.float64)
    scale = gamma / np.sqrt(var + eps)
    return (w * scale.reshape(-1, *([1] * (w.ndim - 1)))).astype(np.float32), ((b - mean) * scale + beta).astype(np.float32)
