"""A Network.run() of Input -> Conv2dConnection [PostPre or no rule] -> LIFNodes, stepped through the CPU oracle's operators only.

network.py's loop body per timestep (reference network.py:380-461):
  1. the connection's current from the input layer's spikes of the PREVIOUS step (oracle.prop_conv2d),
  2. the input layer takes this step's spikes and updates its trace (oracle.input_step),
  3. the LIF step (oracle.lif_step),
  4. with learning on, PostPre on the convolution (oracle.conv2d_postpre, learning.py:457-497).
Every constant (decays, thresholds, trace parameters, rates, bounds, weight decay) is read from the built layer and connection
objects.  State -- the input layer's last spikes included, which the next run's first convolution reads -- carries across
consecutive run() calls, like the network's own.  Independent of every device plan: what the conv plans are checked against.
"""
import numpy as np
import torch

import oracle

f32, u8 = np.float32, np.uint8


def _scalar(t):
    if isinstance(t, torch.Tensor):
        assert t.numel() == 1, "per-neuron parameters are outside this helper"
        return float(t.detach().cpu().reshape(()))
    return float(t)


def _host(t, dtype):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(dtype))


class ConvOracleRun:
    """`net` holds layers "X" (Input, traces on) and "Y" (LIFNodes) and the connection ("X", "Y") (Conv2dConnection).  The state is
    taken from the layers when they are already sized for batch `B`, otherwise it is the state set_batch_size() would give."""

    def __init__(self, net, B):
        X, Y, c = net.layers["X"], net.layers["Y"], net.connections[("X", "Y")]
        assert X.traces, "the input layer must keep a trace (PostPre reads it)"
        assert c.norm is None, "weight normalisation is outside this helper"
        self.B, self.src_shape, self.tgt_shape = B, tuple(X.shape), tuple(Y.shape)
        self.stride, self.pad = c.stride[0], c.padding[0]
        self.bias = _host(c.b, f32)
        self.W = _host(c.w, f32)
        self.x_params = dict(trace_decay=_scalar(X.trace_decay), trace_scale=_scalar(X.trace_scale), additive=bool(X.traces_additive))
        self.lif_params = dict(decay=_scalar(Y.decay), rest=_scalar(Y.rest), reset=_scalar(Y.reset), thresh=_scalar(Y.thresh),
                               refrac0=_scalar(Y.refrac), dt=_scalar(Y.dt),
                               lbound=None if Y.lbound is None else _scalar(Y.lbound))
        self.y_traces = bool(Y.traces)
        if self.y_traces:
            self.lif_params.update(trace_decay=_scalar(Y.trace_decay), trace_scale=_scalar(Y.trace_scale), additive=bool(Y.traces_additive))
        rule = c.update_rule
        self.rule = None
        if rule is not None and type(rule).__name__ == "PostPre":
            lo, hi = rule._bounds()
            self.rule = dict(nu0=f32(float(rule.nu[0])), nu1=f32(float(rule.nu[1])), decay=f32(float(rule.weight_decay)), wmin=lo, wmax=hi)
        else:
            assert rule is None or type(rule).__name__ == "NoOp", type(rule).__name__
        nX, nY = (B,) + self.src_shape, (B,) + self.tgt_shape
        if tuple(Y.v.shape) == nY and tuple(X.s.shape) == nX:
            self.sX = _host(X.s, u8)
            self.xX = _host(X.x, f32)
            self.v, self.r = _host(Y.v, f32), _host(Y.refrac_count, f32)
            self.sY = _host(Y.s, u8)
            self.xY = _host(Y.x, f32) if self.y_traces else None
        else:
            self.sX, self.xX = np.zeros(nX, u8), np.zeros(nX, f32)
            self.v = np.full(nY, self.lif_params["rest"], f32)
            self.r = np.zeros(nY, f32)
            self.sY = np.zeros(nY, u8)
            self.xY = np.zeros(nY, f32) if self.y_traces else None

    def run(self, spikes, learning=True, voltages=False):
        """spikes [T, B, Cin, H, W] (uint8; values above 1 count as that many in the convolution and the rule).  Returns the raster
        [T, B, Cout, OH, OW], the voltage raster when asked, and copies of the state after the run."""
        spikes = np.ascontiguousarray(spikes, dtype=u8)
        T = spikes.shape[0]
        assert spikes.shape[1:] == (self.B,) + self.src_shape, spikes.shape
        learn = learning and self.rule is not None
        ras = np.zeros((T, self.B) + self.tgt_shape, u8)
        vras = np.zeros((T, self.B) + self.tgt_shape, f32) if voltages else None
        for t in range(T):
            I = oracle.prop_conv2d(self.W, self.sX, self.bias, stride=self.stride, pad=self.pad)
            self.sX = np.ascontiguousarray(spikes[t])
            oracle.input_step(self.sX, self.xX, **self.x_params)
            oracle.lif_step(self.v, self.r, self.sY, self.xY, I, **self.lif_params)
            if learn:
                oracle.conv2d_postpre(self.W, self.sX, self.xX, self.sY, self.xY, stride=self.stride, pad=self.pad, **self.rule)
            ras[t] = self.sY
            if voltages:
                vras[t] = self.v
        out = dict(s=ras, v=self.v.copy(), refrac_count=self.r.copy(), sY=self.sY.copy(), xX=self.xX.copy(), W=self.W.copy())
        if self.y_traces:
            out["xY"] = self.xY.copy()
        if voltages:
            out["vras"] = vras
        return out
