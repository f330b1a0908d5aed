"""Network.layer_major on the host: the attribute and ann_to_snn's argument exist, and a network on CPU tensors ignores the request --
it runs the plain-PyTorch step loop (`host-torch`) and gives what the same network gives without it."""
import warnings

import torch
import torch.nn as nn

from layer_major_cases import build, spike_input, weights


def test_the_attribute_and_the_conversion_argument():
    from bindsnet_amd.conversion import ann_to_snn
    from bindsnet_amd.network import Network
    assert Network().layer_major is False
    ann = nn.Sequential(nn.Linear(6, 4), nn.ReLU(), nn.Linear(4, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert ann_to_snn(ann, (6,)).layer_major is False
        assert ann_to_snn(ann, (6,), layer_major=True).layer_major is True


def test_a_host_network_ignores_the_request():
    spec = ((3, 6, 6), [("conv", 5, 3, 1, 1), ("pool",), ("fc", 4)])
    ws, x = weights(spec, 3, grid=False), spike_input(spec, 6, 2, 4)
    seen = []
    for lm in (True, False):
        net = build(spec, ws, 2, lm)
        net.run({"0": x.clone()}, time=6)
        seen.append((net.last_plan, [(l.s.clone(), l.v.clone()) for n, l in net.layers.items() if n != "0"], net.layers["3"].summed.clone()))
    assert seen[0][0] == seen[1][0] == "host-torch"
    assert bool(seen[1][2].ne(0).any())
    assert torch.equal(seen[0][2], seen[1][2])
    for (s, v), (s0, v0) in zip(seen[0][1], seen[1][1]):
        assert torch.equal(s, s0) and torch.equal(v, v0)
