"""What the layer-major tests share: a chain network built from a short spec, and its plain float64 reference.

A spec is (input shape, [("conv", cout, k, stride, pad) | ("pool",) | ("fc", n)]).  `grid=True` puts every weight and bias on a 1/64 grid
with small integer numerators (threshold 1, 2x2 pooling, inputs 0 / 1 / 2 or multiples of 1/4): every partial sum is then exact in
float32 in any order (tests/conv_wide_cases.py's device), so the float64 result is the only correct one and equality is exact."""
import numpy as np
import torch
import torch.nn.functional as F


def shapes(spec):
    shape, out = tuple(spec[0]), []
    for op in spec[1]:
        if op[0] == "conv":
            _, cout, k, s, p = op
            shape = (cout, (shape[1] + 2 * p - k) // s + 1, (shape[2] + 2 * p - k) // s + 1)
        elif op[0] == "pool":
            shape = (shape[0], shape[1] // 2, shape[2] // 2)
        else:
            shape = (op[1],)
        out.append(shape)
    return out


def weights(spec, seed, grid):
    """[(w, b) or None] per op: conv w [Cout, Cin, k, k], fc w [n_in, n_out]."""
    rng, prev, out = np.random.default_rng(seed), tuple(spec[0]), []
    for op, shape in zip(spec[1], shapes(spec)):
        if op[0] == "pool":
            out.append(None)
        else:
            wshape = (op[1], prev[0], op[2], op[2]) if op[0] == "conv" else (int(np.prod(prev)), op[1])
            fan = int(np.prod(wshape[1:])) if op[0] == "conv" else wshape[0]
            if grid:                                   # numerators in [-4, 12]: a mean of 4/64 per tap, about one threshold per 16 active taps
                w, b = rng.integers(-4, 13, wshape) / 64.0, rng.integers(-8, 9, wshape[0] if op[0] == "conv" else wshape[1]) / 64.0
            else:
                w, b = rng.standard_normal(wshape) * 2.0 / np.sqrt(fan) + 0.5 / fan, rng.standard_normal(shape[0]) * 0.1
            out.append((torch.from_numpy(w.astype(np.float32)), torch.from_numpy(b.astype(np.float32))))
        prev = shape
    return out


def build(spec, ws, B, layer_major, refrac=0, lbound=None, traces=False, extra=None):
    """The chain as a bindsnet_amd Network (on the host; the caller moves it).  The last layer has sum_input."""
    from bindsnet_amd.conversion import SubtractiveResetIFNodes
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input
    from bindsnet_amd.network.topology import AvgPool2dConnection, Connection, Conv2dConnection
    net = Network(batch_size=B)
    net.layer_major = layer_major
    prev = Input(shape=spec[0])
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
        prev = layer
    if extra is not None:
        extra(net)
    return net


def reference(spec, ws, x, state, refrac=0, lbound=None):
    """One run of the chain in float64, step by step: layer k at step t reads layer k-1's spikes of step t-1.  x [T, B, *shape]; `state`
    (a dict, {} before the first run) carries every layer's s, v, refrac_count, summed from run to run.  Returns the trains [T, B, *shape]."""
    T, B = x.shape[:2]
    n = len(spec[1])
    if not state:
        state.update(s=[torch.zeros(B, *spec[0], dtype=torch.float64)] + [torch.zeros(B, *sh, dtype=torch.float64) for sh in shapes(spec)],
                     v=[torch.zeros(B, *sh, dtype=torch.float64) for sh in shapes(spec)],
                     rc=[torch.zeros(B, *sh, dtype=torch.float64) for sh in shapes(spec)], summed=torch.zeros(B, *shapes(spec)[-1], dtype=torch.float64))
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
            v, rc = state["v"][k], state["rc"][k]
            v += (rc == 0).double() * cur
            rc.copy_((rc > 0).double() * (rc - 1.0))
            s = v >= 1.0
            rc[s] = float(refrac)
            v[s] -= 1.0
            if lbound is not None:
                v.clamp_(min=lbound)
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
