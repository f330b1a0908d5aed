"""`ann_to_snn`: a trained torch.nn model as a spiking Network (reference: bindsnet/conversion/conversion.py).  Host code; the
network it returns runs on the device after `network.to("cuda")`: every layer and connection it is made of has a kernel.

What it builds, child by child of the model (a top-level Sequential is opened up, one level):
    Linear          -> `node_type` layer of out_features neurons behind a Connection with w = weight.t() and b = bias (zeros without)
    Conv2d          -> `node_type` layer (out_channels, OH, OW) behind a Conv2dConnection with the module's w and b
    MaxPool2d       -> PassThroughNodes behind a MaxPool2dConnection(decay=1)
    Permute         -> PassThroughNodes behind a PermuteConnection
    ConstantPad2d   -> PassThroughNodes behind a ConstantPad2dConnection
    AvgPool2d       -> `node_type` layer (C, OH, OW) behind an AvgPool2dConnection with the module's parameters: the usual spiking
                       pooling layer -- an IF neuron fed count / k^2 fires at the mean rate of its window (not in the reference)
    AdaptiveAvgPool2d -> the same, with kernel = stride = in // out, where every input size is a multiple of its output size (a
                       None entry keeps that size); NotImplementedError naming both sizes otherwise
    BatchNorm2d behind a Conv2d, BatchNorm1d behind a Linear -> folded into that layer's weights and bias first (`fold_batchnorm`,
                       on the deep copy, before data_based_normalization) and replaced by nn.Identity, so no position moves; a
                       BatchNorm anywhere else raises NotImplementedError, one without running statistics ValueError
    anything else   -> skipped (ReLU is what the spiking neurons themselves stand for; Flatten, Dropout and Identity change nothing
                       a spiking layer would see)
The layers are named "Input", "1", "2", ... after the child's position, so a skipped child leaves a gap, and a connection's key
is (str(i - 1), str(i)) whether or not a layer of that name exists.  Every `node_type` layer gets reset=0, thresh=1, refrac=0;
the last one sum_input=True -- its `summed` is the network's readout.  Only SubtractiveResetIFNodes takes sum_input here, so any
other `node_type` raises NotImplementedError at the last layer.

Kept from the reference as it is, not repaired: the output shape of a Permute child is looked up in the previous layer's shape
with the batch-inclusive dims; a Conv2d without bias gets zeros(layer.shape[1]), one per output ROW; a ConstantPad2d's height
grows by padding[0] + padding[1], the left and right pads.  Where the resulting graph cannot run, the run raises before it
changes any state.  `torch.load` of a path is called as the reference calls it.

How to drive it: `data_based_normalization` scales every layer by percentiles of the ANN's real-valued activations, so the network
is meant to be fed the real-valued sample itself at every step (encoding.repeat / `image.repeat(time, ...)`), not a Poisson train.
That analog input -- a float32 [T, B, *shape] entry of `inputs` -- runs on the device where the first child is a Linear or a Conv2d
(csrc/snn_real.hip: the ordered dense product and convolution over real values, include/snnhip.h f17); uint8 / bool spike trains
run as before, and float32 zeros and ones give the bits their bytes give.

On the device the limits of the parts apply: Conv2d with dilation 1, symmetric stride and padding; an analog input into a
PermuteConnection or ConstantPad2dConnection (a first child Permute / ConstantPad2d) raises; no
fused plan (`network.last_plan == "generic"`); no monitor on `summed`.  A Conv2d with more than 16 input channels runs in the stated
order of snn_prop_conv2d_f32 (include/snnhip.h): equal to the reference bit for bit where every partial sum is exact, else up to
summation rounding."""
import warnings
from copy import deepcopy
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn
from torch.nn.modules.utils import _pair

from ..network import Network
from ..network import nodes, topology
from .nodes import PassThroughNodes, SubtractiveResetIFNodes
from .topology import ConstantPad2dConnection, PermuteConnection


class Permute(nn.Module):
    """`x.permute(*dims)` as a module, so that a Sequential (and `ann_to_snn`) can see it."""

    def __init__(self, dims):
        super().__init__()
        self.dims = dims

    def forward(self, x):
        return x.permute(*self.dims).contiguous()


class FeatureExtractor(nn.Module):
    """Runs `submodule`'s children one after the other and keeps every child's output: {"input": x, child name: activation}.
    The input of a Linear child is flattened to [-1, in_features] first."""

    def __init__(self, submodule):
        super().__init__()
        self.submodule = submodule

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        seen = {"input": x}
        for name, child in self.submodule._modules.items():
            if isinstance(child, nn.Linear):
                x = x.view(-1, child.in_features)
            x = child(x)
            seen[name] = x
        return seen


def _is_weighted(module) -> bool:
    return isinstance(module, (nn.Linear, nn.Conv2d))


def data_based_normalization(ann: Union[nn.Module, str], data: torch.Tensor, percentile: float = 99.9):
    """Rescale the weights and biases of `ann` IN PLACE so that the `percentile`-th percentile of every ReLU's activations on
    `data` becomes 1, and return it.  A path is read with torch.load.

    The control flow is the reference's, quirks included: the model's top-level children are walked once; inside a Sequential
    child every ReLU rescales the weighted layer seen last (by `previous factor / this factor`, the bias by `1 / this factor`);
    a top-level Linear is rescaled like a ReLU would rescale -- with whatever activations were looked at last -- and never
    becomes the "weighted layer seen last" itself; a top-level ReLU or Conv2d behaves as inside a Sequential."""
    if isinstance(ann, str):
        ann = torch.load(ann)
    assert isinstance(ann, nn.Module)
    for param in ann.parameters():
        param.requires_grad = False
    outer = FeatureExtractor(ann).forward(data)

    state = {"last": None, "factor": 1}

    def rescale(acts) -> None:
        last = state["last"]
        if last is None:
            return
        scale = np.percentile(acts.cpu(), percentile)
        last.weight *= state["factor"] / scale
        last.bias /= scale
        state["factor"] = scale

    for name, module in ann._modules.items():
        if isinstance(module, nn.Sequential):
            inner = FeatureExtractor(module).forward(data)
            for inner_name, module in module.named_children():      # (`module` is the LAST inner child behind this loop, as there)
                activations = inner[inner_name]
                if isinstance(module, nn.ReLU):
                    rescale(activations)
                elif _is_weighted(module):
                    state["last"] = module
        if isinstance(module, nn.Linear):
            if state["last"] is not None:
                rescale(activations)                               # (the activations looked at last, whichever child's they were)
        else:
            activations = outer[name]
            if isinstance(module, nn.ReLU):
                rescale(activations)
            elif _is_weighted(module):
                state["last"] = module
    return ann


def _flat_children(ann):
    """(container, name, child) of every child `ann_to_snn` sees, in its order: a top-level Sequential is opened up, one level."""
    found = []
    for name, child in ann.named_children():
        if isinstance(child, nn.Sequential):
            found += [(child, inner, grandchild) for inner, grandchild in child.named_children()]
        else:
            found.append((ann, name, child))
    return found


def fold_batchnorm(ann: nn.Module) -> nn.Module:
    """Fold every BatchNorm2d directly behind a Conv2d, and every BatchNorm1d directly behind a Linear, into that layer IN PLACE and
    put nn.Identity where it stood, so that every child keeps its position (and `ann_to_snn` its layer names); returns `ann`.
    Inference statistics, computed in float64 and cast to float32 once:
        scale = gamma / sqrt(running_var + eps);  w' = w * scale per output channel;  b' = (b - running_mean) * scale + beta
    with b = 0 where the layer had no bias (it gains one) and gamma = 1, beta = 0 for affine=False.  A BatchNorm without running
    statistics raises ValueError, one that is not directly behind its weighted layer NotImplementedError, both naming the child;
    "directly behind" is the previous child as `ann_to_snn` walks them.  A model without BatchNorm is left as it is."""
    before = None
    for position, (owner, name, child) in enumerate(_flat_children(ann), start=1):
        if isinstance(child, nn.modules.batchnorm._BatchNorm):
            what = f"{type(child).__name__} child '{name}' (position {position})"
            if child.running_mean is None or child.running_var is None:
                raise ValueError(f"fold_batchnorm: {what} has no running statistics (track_running_stats=False): there is nothing "
                                 "to fold at inference")
            takes = (isinstance(child, nn.BatchNorm2d) and isinstance(before, nn.Conv2d)) or \
                    (isinstance(child, nn.BatchNorm1d) and isinstance(before, nn.Linear))
            if not takes:
                raise NotImplementedError(f"fold_batchnorm: {what} is not directly behind a {'Conv2d' if isinstance(child, nn.BatchNorm2d) else 'Linear'}"
                                          f" (the child before it is {type(before).__name__ if before is not None else 'none'}); only a "
                                          "BatchNorm2d behind a Conv2d and a BatchNorm1d behind a Linear can be folded")
            with torch.no_grad():
                f64 = lambda t: t.detach().to(torch.float64)      # noqa: E731
                w = f64(before.weight)
                n = w.shape[0]
                scale = (f64(child.weight) if child.weight is not None else torch.ones(n, dtype=torch.float64)) / \
                    torch.sqrt(f64(child.running_var) + child.eps)
                b = f64(before.bias) if before.bias is not None else torch.zeros(n, dtype=torch.float64)
                beta = f64(child.bias) if child.bias is not None else torch.zeros(n, dtype=torch.float64)
                b = (b - f64(child.running_mean)) * scale + beta
                before.weight.copy_((w * scale.view(-1, *([1] * (w.dim() - 1)))).to(torch.float32))
                folded = b.to(dtype=torch.float32, device=before.weight.device)
                if before.bias is None:
                    before.bias = nn.Parameter(folded, requires_grad=before.weight.requires_grad)
                else:
                    before.bias.copy_(folded)
            child = nn.Identity()
            setattr(owner, name, child)
        before = child
    return ann


def _avgpool_output(prev, kernel_size, stride, padding, ceil_mode):
    """(rows, columns) of an average pooling behind `prev`, as torch computes them (what F.avg_pool2d refuses raises here)."""
    probe = torch.nn.functional.avg_pool2d(torch.empty(1, *prev.shape, device="meta"), kernel_size=kernel_size, stride=stride,
                                           padding=padding, ceil_mode=ceil_mode)
    return tuple(probe.shape[2:])


def _conv_output(prev, module):
    """(rows, columns) of a Conv2d / MaxPool2d output as the reference computes them: float division, then int()."""
    k, p, s = module.kernel_size, module.padding, module.stride
    return (int((prev.shape[1] - k[0] + 2 * p[0]) / s[0] + 1), int((prev.shape[2] - k[1] + 2 * p[1]) / s[1] + 1))


def _ann_to_snn_helper(prev, current, node_type, last=False, **kwargs):
    """(layer, connection) for the ANN module `current` behind the spiking layer `prev`, or (None, None) for a module that has no
    spiking counterpart."""
    spiking = dict(reset=0, thresh=1, refrac=0, sum_input=last, **kwargs)
    if isinstance(current, nn.Linear):
        layer = node_type(n=current.out_features, **spiking)
        bias = current.bias if current.bias is not None else torch.zeros(layer.n)
        # (a transposed view, as in the reference -- on the host MKL is then handed the same operand; Connection stores it contiguously
        #  once it moves to the device, where the kernels read [in, out] row-major)
        # (prop_auto: the IF layers of a converted network fire at their normalised rates, densely -- the product's body is chosen on the device)
        return layer, topology.Connection(source=prev, target=layer, w=current.weight.t(), b=bias, prop_auto=True)
    if isinstance(current, nn.Conv2d):
        layer = node_type(shape=(current.out_channels, *_conv_output(prev, current)), **spiking)
        bias = current.bias if current.bias is not None else torch.zeros(layer.shape[1])
        return layer, topology.Conv2dConnection(source=prev, target=layer, kernel_size=current.kernel_size, stride=current.stride,
                                                padding=current.padding, dilation=current.dilation, w=current.weight, b=bias)
    if isinstance(current, nn.MaxPool2d):
        current.kernel_size, current.padding, current.stride = _pair(current.kernel_size), _pair(current.padding), _pair(current.stride)
        layer = PassThroughNodes(shape=(prev.shape[0], *_conv_output(prev, current)))
        return layer, topology.MaxPool2dConnection(source=prev, target=layer, kernel_size=current.kernel_size, stride=current.stride,
                                                   padding=current.padding, dilation=current.dilation, decay=1)
    if isinstance(current, (nn.AvgPool2d, nn.AdaptiveAvgPool2d)):
        if len(prev.shape) != 3:
            raise NotImplementedError(f"ann_to_snn: {type(current).__name__} behind a layer of shape {tuple(prev.shape)}: average pooling "
                                      "needs a (C, H, W) layer in front of it")
        if isinstance(current, nn.AdaptiveAvgPool2d):
            size, plane = current.output_size, tuple(prev.shape[1:])
            want = tuple(size) if isinstance(size, (tuple, list)) else (size, size)
            want = tuple(i if o is None else int(o) for i, o in zip(plane, want))
            if len(want) != 2 or min(want) <= 0 or any(i % o for i, o in zip(plane, want)):
                raise NotImplementedError(f"ann_to_snn: AdaptiveAvgPool2d from an input of size {plane} to an output of size {want}: only "
                                          "input sizes that are multiples of the output sizes are supported (its windows then all "
                                          "have the same size: kernel = stride = in // out)")
            pool = dict(kernel_size=tuple(i // o for i, o in zip(plane, want)))
            pool["stride"] = pool["kernel_size"]
        else:
            pool = dict(kernel_size=_pair(current.kernel_size), stride=_pair(current.kernel_size if current.stride is None else current.stride),
                        padding=_pair(current.padding), ceil_mode=current.ceil_mode, count_include_pad=current.count_include_pad,
                        divisor_override=current.divisor_override)
        rows, columns = _avgpool_output(prev, pool["kernel_size"], pool["stride"], pool.get("padding", 0), pool.get("ceil_mode", False))
        layer = node_type(shape=(prev.shape[0], rows, columns), **spiking)
        return layer, topology.AvgPool2dConnection(source=prev, target=layer, **pool)
    if isinstance(current, Permute):
        layer = PassThroughNodes(shape=[prev.shape[current.dims[k]] for k in range(3)])
        return layer, PermuteConnection(source=prev, target=layer, dims=current.dims)
    if isinstance(current, nn.ConstantPad2d):
        pad = current.padding
        layer = PassThroughNodes(shape=[prev.shape[0], pad[0] + pad[1] + prev.shape[1], pad[2] + pad[3] + prev.shape[2]])
        return layer, ConstantPad2dConnection(source=prev, target=layer, padding=pad)
    return None, None


def ann_to_snn(ann: Union[nn.Module, str], input_shape: Sequence[int], data: Optional[torch.Tensor] = None, percentile: float = 99.9,
               node_type: Optional[nodes.Nodes] = SubtractiveResetIFNodes, **kwargs) -> Network:
    """The spiking Network of the module docstring for `ann` (a deep copy is converted; a path is read with torch.load).  BatchNorm
    children are folded into the copy first (`fold_batchnorm`).  With
    `data` the copy's weights are rescaled by data_based_normalization first; without it a RuntimeWarning says they are not.
    `kwargs` go to every `node_type` layer."""
    ann = torch.load(ann) if isinstance(ann, str) else deepcopy(ann)
    assert isinstance(ann, nn.Module)
    ann = fold_batchnorm(ann)                          # (nothing to do, and nothing done, for a model without BatchNorm)
    if data is None:
        warnings.warn("Data is None. Weights will not be scaled.", RuntimeWarning)
    else:
        ann = data_based_normalization(ann=ann, data=data.detach(), percentile=percentile)

    snn = Network()
    prev = nodes.Input(shape=input_shape)
    snn.add_layer(prev, name="Input")

    children = []
    for child in ann.children():
        children += list(child.children()) if isinstance(child, nn.Sequential) else [child]

    for i, current in enumerate(children[:-1], start=1):
        layer, connection = _ann_to_snn_helper(prev, current, node_type, **kwargs)
        if layer is None or connection is None:
            continue
        snn.add_layer(layer, name=str(i))
        snn.add_connection(connection, source=str(i - 1), target=str(i))
        prev = layer

    i = len(children)                                  # (the reference counts the last child too, a one-child model included)
    layer, connection = _ann_to_snn_helper(prev, children[-1], node_type, last=True, **kwargs)
    if layer is not None or connection is not None:
        snn.add_layer(layer, name=str(i))
        snn.add_connection(connection, source=str(i - 1), target=str(i))
    return snn
