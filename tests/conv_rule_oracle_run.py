"""Hebbian / WeightDependentPostPre on a Conv2dConnection through the CPU oracle: conv_oracle_run.ConvOracleRun's stepping with the
rule's own apply step.

The two batch-reduced sums come from the unmodified oracle.conv2d_postpre on a ZERO weight tensor, without decay or clamp: with
(nu0, nu1) = (1, 0) it leaves 0 - 1 * pre, with (0, 1) it leaves 0 + 1 * post -- both exact, so `pre = 0 - (0 - pre)` and `post` are
the oracle's sums bit for bit (positions ascending per sample, then ATen's sum(dim=0) order over the batch).  The rule's statements
(learning.py:1372-1380 / :950-976, then LearningRule.update :87-104) follow in numpy float32, one rounding per operation."""
from types import SimpleNamespace

import numpy as np

import oracle
from conv_oracle_run import ConvOracleRun

f32 = np.float32


def conv_sums(shape, sX, xX, sY, xY, stride, pad):
    """(pre, post), each shaped like the weights."""
    neg_pre, post = np.zeros(shape, f32), np.zeros(shape, f32)
    oracle.conv2d_postpre(neg_pre, sX, xX, sY, xY, stride=stride, pad=pad, nu0=f32(1.0), nu1=f32(0.0))
    oracle.conv2d_postpre(post, sX, xX, sY, xY, stride=stride, pad=pad, nu0=f32(0.0), nu1=f32(1.0))
    return np.subtract(f32(0.0), neg_pre, dtype=f32), post


def apply_rule(W, pre, post, *, weight_dependent, nu0, nu1, decay=1.0, wmin=None, wmax=None):
    """In place on W (float32)."""
    nu0, nu1, decay = f32(nu0), f32(nu1), f32(decay)
    w = W
    if not weight_dependent:
        w = w + nu0 * pre
        w = w + nu1 * post
    else:
        lo, hi = f32(wmin), f32(wmax)
        upd = np.zeros_like(W)
        if nu0 != 0:
            upd = upd - (nu0 * pre) * (w - lo)
        if nu1 != 0:
            upd = upd + (nu1 * post) * (hi - w)
        w = w + upd
    w = w * decay
    if wmin is not None:
        w = np.where(w < f32(wmin), f32(wmin), w)
    if wmax is not None:
        w = np.where(w > f32(wmax), f32(wmax), w)
    assert w.dtype == f32
    W[...] = w


class ConvRuleOracleRun(ConvOracleRun):
    """`net` as for ConvOracleRun, the connection's rule being Hebbian or WeightDependentPostPre."""

    def __init__(self, net, B):
        c = net.connections[("X", "Y")]
        rule = c.update_rule
        assert type(rule).__name__ in ("Hebbian", "WeightDependentPostPre"), type(rule).__name__
        bare = SimpleNamespace(stride=c.stride, padding=c.padding, b=c.b, w=c.w, norm=c.norm, update_rule=None)
        super().__init__(SimpleNamespace(layers=net.layers, connections={("X", "Y"): bare}), B)
        lo, hi = rule._bounds()
        self.hebb = dict(weight_dependent=type(rule).__name__ == "WeightDependentPostPre", nu0=float(rule.nu[0]), nu1=float(rule.nu[1]),
                         decay=float(rule.weight_decay), wmin=lo, wmax=hi)

    def run(self, spikes, learning=True):
        spikes = np.ascontiguousarray(spikes, dtype=np.uint8)
        T = spikes.shape[0]
        ras = np.zeros((T, self.B) + self.tgt_shape, np.uint8)
        for t in range(T):
            I = oracle.prop_conv2d(self.W, self.sX, self.bias, stride=self.stride, pad=self.pad)
            self.sX = np.ascontiguousarray(spikes[t])
            oracle.input_step(self.sX, self.xX, **self.x_params)
            oracle.lif_step(self.v, self.r, self.sY, self.xY, I, **self.lif_params)
            if learning:
                pre, post = conv_sums(self.W.shape, self.sX, self.xX, self.sY, self.xY, self.stride, self.pad)
                apply_rule(self.W, pre, post, **self.hebb)
            ras[t] = self.sY
        return dict(s=ras, v=self.v.copy(), refrac_count=self.r.copy(), sY=self.sY.copy(), xX=self.xX.copy(), xY=self.xY.copy(), W=self.W.copy())
