"""The matrix-core convolution's interface on the CPU: the entry point refuses bad arguments and shapes beyond its limits before any
launch, the predicate is a fact of shape and request, the host path ignores prop_auto, ann_to_snn asks for its convolutions."""
import torch

INVALID, UNSUPPORTED = -1, -2
OK = dict(B=1, Cin=17, H=5, Wd=5, Cout=5, KH=3, KW=3, stride=1, pad=1)


def _call(W=1, s=1, out=1, **kw):
    from bindsnet_amd import _lib
    return _lib.lib().snn_prop_conv2d_mfma_f32(W, None, s, out, *dict(OK, **kw).values(), 0, None, None)


def test_entry_point_refuses_before_any_launch_and_the_predicate_follows_the_shape():
    assert _call(W=None) == _call(s=None) == _call(out=None) == INVALID
    for key, bad in (("B", 0), ("Cin", 0), ("H", 0), ("Wd", 0), ("Cout", 0), ("KH", 0), ("KW", 8), ("stride", 0), ("pad", -1)):
        assert _call(**{key: bad}) == INVALID, (key, bad)
    # the int limits of snn_prop_conv2d_f32 (taps, image), the padded tap count (1 channel counts as 16), the grid
    assert _call(Cin=1 << 20, KH=50, KW=50, H=50, Wd=50, pad=0) == UNSUPPORTED
    assert _call(H=1 << 16, Wd=1 << 16, KH=1, KW=1, pad=0) == UNSUPPORTED
    assert _call(Cin=1, H=1 << 14, Wd=1 << 14, KH=1 << 14, KW=1 << 14, pad=0) == UNSUPPORTED
    assert _call(B=1 << 20, H=32, Wd=32) == UNSUPPORTED                           # 2^24 blocks of 64 output pixels
    assert _call(H=4, Wd=758) == UNSUPPORTED                                      # the LDS limit, below
    from bindsnet_amd.ops import conv2d_mfma_takes as takes
    wide = (64, 8, 8, 128, 3, 3, 1, 1)
    assert takes(1, *wide) and takes(16, *wide) and not takes(1, *wide, asked=False) and not takes(0, *wide)
    assert not takes(1, 16, 8, 8, 32, 3, 3, 1, 1) and takes(2, 4, 9, 9, 300, 7, 7, 1, 0)      # k_conv2d's shapes; a bank beyond 64 KiB
    assert takes(1, 17, 4, 757, 5, 3, 3, 1, 1) and not takes(1, 17, 4, 758, 5, 3, 3, 1, 1)     # 8192 + 192 Wd <= 153600


def test_the_host_path_ignores_the_request_and_ann_to_snn_asks():
    from torch import nn
    from bindsnet_amd.conversion import ann_to_snn
    from bindsnet_amd.network.nodes import IFNodes, Input
    from bindsnet_amd.network.topology import Conv2dConnection
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(8, 20, 3, 3, generator=g), torch.randn(8, generator=g)
    plain, asked = (Conv2dConnection(Input(shape=(20, 6, 6)), IFNodes(shape=(8, 6, 6)), kernel_size=3, padding=1, w=w.clone(), b=b.clone(),
                                     prop_auto=ask) for ask in (False, True))
    s = (torch.rand(2, 20, 6, 6, generator=g) < 0.3).to(torch.uint8)
    assert plain.prop_auto is False and asked.prop_auto is True and torch.equal(plain.compute(s), asked.compute(s))
    asked.reset_prop_stats()
    assert asked.prop_stats() == plain.prop_stats() == {"matrix_tiles": 0, "event_tiles": 0}
    net = ann_to_snn(nn.Sequential(nn.Conv2d(3, 20, 3, padding=1), nn.ReLU(), nn.Conv2d(20, 8, 3, padding=1), nn.ReLU()), input_shape=(3, 6, 6))
    convs = [c for c in net.connections.values() if isinstance(c, Conv2dConnection)]
    assert len(convs) == 2 and all(c.prop_auto is True for c in convs)
