"""Network.run() for networks that live on the HOST: a plain-PyTorch step loop with the reference's semantics.

The product of this package is the MI355X path (csrc/*.hip behind the C ABI); this module exists so that the drop-in
package still constructs and runs where there is no GPU (SURVEY.md 8(b) fallback rule) -- a laptop, a CI box -- and it is a
second, independent statement of the same semantics: tests/test_host_path.py pins it to the reference-generated fixtures
the GPU tests use.  It is selected by Network.run only when the network's tensors are CPU tensors; it never touches
libsnnhip and has nothing to do with oracle/ (test infrastructure).  Supported on this path: Input / LIFNodes /
DiehlAndCookNodes / AdaptiveLIFNodes / McCullochPitts / IFNodes / BoostedLIFNodes / CurrentLIFNodes / IzhikevichNodes / SRM0Nodes / CSRMNodes; MulticompartmentConnection + Weight (no rule / PostPre / MSTDP / MSTDPET), Connection and LocalConnection (no
rule / PostPre / MSTDP / Hebbian / WeightDependentPostPre / MSTDPET / Rmax), Conv2dConnection (no rule / PostPre / MSTDP at batch 1);
clamp / unclamp / injects_v / masks / one_step / reward; Monitor / NetworkMonitor.

What each function states (paths inside BindsNET): network.py:211-250,380-465 (loop, `zeros + c1 + c2` accumulation,
normalise), nodes.py:96-107,211-221,500-529,1069-1111 (layers), topology.py:332-346,437-479,799-815 and
topology_features.py:633-645 (propagation), MCC_learning.py:224-302,86-110 / learning.py:390-420,1504-1574,87-104 (rules).
Per-step cost is the reference's (one ATen call per operation): this path is for function, not speed.
"""
from typing import Dict

import torch
import torch.nn.functional as F

from .. import _lib


def aten_sum_leaves_serial_order(outer: int, n_reduced: int, n_cols: int, threads: int) -> bool:
    """True when torch.sum over the middle dimension of a contiguous float [outer, n_reduced, n_cols] tensor (outer = 1: also
    sum(dim=0) of [n_reduced, n_cols]) at `threads` intra-op threads sums the last n_cols mod 32 columns in another order than it
    does serially.  The reference's own float sums are not independent of the thread count: reductions of at least 32768
    elements are split over the outermost non-reduced dimension that has `threads` entries (if neither has: the larger one,
    ties to the outer) -- and when that is the COLUMNS, cut into `threads` ranges of c = ceil(n_cols / threads) whose ends are
    rounded down to multiples of 32, a last range holding ONLY the n_cols mod 32 < 8 tail columns is summed by another kernel
    of SumKernel.cpp (scalar_outer_sum: groups of four columns in the cascade order of a full group) than the same columns at
    the end of a longer range (vectorized_outer_sum's row_sum leftover).  E.g. n_cols = 100, batch 1: columns 96-99 at 9 or
    >= 12 threads.  Pinned against torch itself by tests/test_aten_sum_threads.py (tools/probe_aten_sum_threads.py prints it)."""
    tail = n_cols % 32
    if threads <= 1 or not 0 < tail < 8:
        return False
    if outer * n_reduced * n_cols < 32768:       # at::internal::GRAIN_SIZE: small reductions run serially
        return False
    if outer >= threads:                         # the outer dimension is split: every slice is summed serially
        return False
    if n_cols < threads and n_cols <= outer:
        return False
    c = -(-n_cols // threads)
    return c * ((n_cols - 1) // c) >= n_cols - tail


def _sum(t, dim):
    """ATen's sum in its SERIAL order, whatever the caller's thread setting: this package pins the serial order (what the
    reference computes with up to 8 threads at the sizes of BASELINE.md, and at any thread count once the batch has at least
    `threads` samples) -- the MI355X kernels, the oracle and, through this helper, the host path.  The thread count is only
    taken down for the call when the model above says the order would change (or the shape is not one it covers)."""
    n = torch.get_num_threads()
    if n == 1:
        return t.sum(dim)
    if t.is_contiguous() and t.dim() in (2, 3) and dim in (0, 1):
        if dim == 0:                                 # [B, ...] over the batch: the trailing dimensions are one run of columns
            shape = (1, t.shape[0], t[0].numel())
        else:
            shape = (t.shape[0], t.shape[1], t.shape[2]) if t.dim() == 3 else None
        if shape is not None and not aten_sum_leaves_serial_order(*shape, n):
            return t.sum(dim)
    torch.set_num_threads(1)
    try:
        return t.sum(dim)
    finally:
        torch.set_num_threads(n)


def _trace_into(layer, s, x) -> None:
    """nodes.py:96-107 on explicit tensors: the trace `x` (in place) after the spikes `s`."""
    x *= layer.trace_decay
    if layer.traces_additive:
        x += layer.trace_scale * s.float()
    else:
        x.masked_fill_(s.bool(), float(layer.trace_scale))


def _trace(layer, s) -> None:
    if layer.traces:
        _trace_into(layer, s, layer.x)


def clamp_mask(spec, n: int) -> torch.Tensor:
    """run(..., clamp= / unclamp=): the reference assigns `s[:, spec] = 1` (network.py:416-429), so `spec` is whatever indexes the
    neuron dimension -- a boolean (or byte) MASK of n entries, or an integer tensor of neuron INDICES (supervised_mnist.py:201-207
    clamps `per_class * label + choice`) -- optionally one row per timestep.  Returns the boolean mask, [n] or [T, n]."""
    m = torch.as_tensor(spec)
    if m.dtype in (torch.bool, torch.uint8) or m.is_floating_point():
        return m.ne(0)
    idx = m.long()
    if idx.dim() <= 1:
        out = torch.zeros(n, dtype=torch.bool, device=idx.device)
        out[idx.reshape(-1)] = True
        return out
    out = torch.zeros(idx.shape[0], n, dtype=torch.bool, device=idx.device)
    out.scatter_(1, idx.reshape(idx.shape[0], -1), True)
    return out


def _step_input(layer, x) -> None:
    layer.s = x                                        # aliases the caller's tensor, like the reference
    _trace(layer, x)


def _lif_membrane(layer, x) -> None:
    """nodes.py:500-526: the LIF step without its trace."""
    layer.v = layer.decay * (layer.v - layer.rest) + layer.rest
    x.masked_fill_(layer.refrac_count > 0, 0.0)        # (in place on the summed input, as the reference does)
    layer.refrac_count -= layer.dt
    layer.v += x
    layer.s = layer.v >= layer.thresh
    layer.refrac_count.masked_fill_(layer.s, float(layer.refrac))
    layer.v.masked_fill_(layer.s, float(layer.reset))
    if layer.lbound is not None:
        layer.v.masked_fill_(layer.v < layer.lbound, float(layer.lbound))


def _step_lif(layer, x) -> None:
    _lif_membrane(layer, x)
    _trace(layer, layer.s)


def _step_mcp(layer, x) -> None:
    """nodes.py:278-288."""
    layer.v = x
    layer.s = layer.v >= layer.thresh
    _trace(layer, layer.s)


def _reset_and_bound(layer, reset) -> None:
    """What the threshold test is followed by in nodes.py:388-393 / :784-789: refractory period, reset, lower bound."""
    layer.refrac_count.masked_fill_(layer.s, layer.refrac)
    layer.v.masked_fill_(layer.s, reset)
    if layer.lbound is not None:
        layer.v.masked_fill_(layer.v < layer.lbound, layer.lbound)


def _step_if(layer, x) -> None:
    """nodes.py:371-395."""
    layer.v += (layer.refrac_count <= 0).float() * x
    layer.refrac_count -= layer.dt
    layer.s = layer.v >= layer.thresh
    _reset_and_bound(layer, layer.reset)
    _trace(layer, layer.s)


def _step_sif(layer, x) -> None:
    """SubtractiveResetIFNodes.forward (conversion/nodes.py:73-99), then the base class's trace and `summed` (nodes.py:96-107)."""
    layer.v += (layer.refrac_count == 0).float() * x
    layer.refrac_count = (layer.refrac_count > 0).float() * (layer.refrac_count - layer.dt)
    layer.s = layer.v >= layer.thresh
    layer.refrac_count.masked_fill_(layer.s, layer.refrac)
    layer.v[layer.s] = layer.v[layer.s] - layer.thresh
    if layer.lbound is not None:
        layer.v.masked_fill_(layer.v < layer.lbound, layer.lbound)
    _trace(layer, layer.s)
    if layer.sum_input:
        layer.summed += x.float()


def _step_boosted(layer, x) -> None:
    """nodes.py:621-648."""
    layer.v *= layer.decay
    x.masked_fill_(layer.refrac_count > 0, 0.0)        # (in place on the summed input, as the reference does)
    layer.refrac_count -= layer.dt
    layer.v += x
    layer.s = layer.v >= layer.thresh
    layer.refrac_count.masked_fill_(layer.s, layer.refrac)
    layer.v.masked_fill_(layer.s, 0)
    _trace(layer, layer.s)


def _step_clif(layer, x) -> None:
    """nodes.py:762-791."""
    layer.v = layer.decay * (layer.v - layer.rest) + layer.rest
    layer.i *= layer.i_decay
    layer.refrac_count -= layer.dt
    layer.i += x
    layer.v += (layer.refrac_count <= 0).float() * layer.i
    layer.s = layer.v >= layer.thresh
    _reset_and_bound(layer, layer.reset)
    _trace(layer, layer.s)


def _step_izh(layer, x) -> None:
    """nodes.py:1265-1296; the lateral sum goes into `x` in place, as in the reference."""
    layer.v = torch.where(layer.s, layer.c, layer.v)
    layer.u = torch.where(layer.s, layer.u + layer.d, layer.u)
    if layer.s.any():
        x += torch.cat([layer.S[:, layer.s[b]].sum(dim=1)[None] for b in range(layer.s.shape[0])], dim=0)
    for _ in range(2):
        layer.v += layer.dt * 0.5 * (0.04 * layer.v ** 2 + 5 * layer.v + 140 - layer.u + x)
    layer.u += layer.dt * layer.a * (layer.b * layer.v - layer.u)
    if layer.lbound is not None:
        layer.v.masked_fill_(layer.v < layer.lbound, layer.lbound)
    layer.s = layer.v >= layer.thresh
    _trace(layer, layer.s)


def _step_srm0(layer, x) -> None:
    """nodes.py:1639-1671, the reference's statements in its order; the draw is torch.rand_like on the global generator."""
    layer.v = layer.decay * (layer.v - layer.rest) + layer.rest
    layer.v += (layer.refrac_count <= 0).float() * layer.eps_0 * x
    layer.rho = layer.rho_0 * torch.exp((layer.v - layer.thresh) / layer.d_thresh)
    layer.s_prob = 1.0 - torch.exp(-layer.rho * layer.dt)
    layer.refrac_count -= layer.dt
    layer.s = torch.rand_like(layer.s_prob) < layer.s_prob
    layer.refrac_count.masked_fill_(layer.s, layer.refrac)
    layer.v.masked_fill_(layer.s, layer.reset)
    if layer.lbound is not None:
        layer.v.masked_fill_(layer.v < layer.lbound, layer.lbound)
    _trace(layer, layer.s)


def _step_csrm(layer, x) -> None:
    """nodes.py:1427-1464, the reference's statements in its order; `x` is the window [B, res_window_size, *shape]."""
    layer.v *= layer.decay
    if layer.learning:
        layer.theta *= layer.theta_decay
    v = torch.einsum("i,kij->kj", layer.resKernel, x)
    v += torch.einsum("i,kij->kj", layer.refKernel, layer.last_spikes)
    layer.v += v.view(x.size(0), *layer.shape)
    layer.s = layer.v >= layer.thresh + layer.theta
    if layer.learning:
        layer.theta += layer.theta_plus * layer.s.float().sum(0)
    layer.last_spikes = torch.cat((layer.last_spikes[:, 1:, :], layer.s[:, None, :]), 1)
    if layer.lbound is not None:
        layer.v.masked_fill_(layer.v < layer.lbound, layer.lbound)
    _trace(layer, layer.s)


def _dc_membrane(layer, x) -> None:
    """nodes.py:1069-1092: everything up to the threshold crossings (left in layer.s) and their reset."""
    layer.v = layer.decay * (layer.v - layer.rest) + layer.rest
    if layer.learning:
        layer.theta *= layer.theta_decay
    layer.v += (layer.refrac_count <= 0).float() * x
    layer.refrac_count -= layer.dt
    layer.s = layer.v >= layer.thresh + layer.theta
    layer.refrac_count.masked_fill_(layer.s, float(layer.refrac))
    layer.v.masked_fill_(layer.s, float(layer.reset))


def _dc_theta(layer, crossings) -> None:
    """nodes.py:1093-1094: every neuron that crossed bumps the shared threshold, summed over the batch `crossings` spans."""
    if layer.learning:
        layer.theta += layer.theta_plus * crossings.float().sum(0)


def _one_spike(s2d) -> None:
    """nodes.py:1097-1105 on a [B, N] bool matrix, in place: one winner per row with a crossing, drawn from the global
    generator (rows in batch order)."""
    if s2d.any():
        rows = s2d.any(1)
        ind = torch.multinomial(s2d.float()[rows], 1)
        rows = rows.nonzero()
        s2d.zero_()
        s2d[rows, ind] = 1


def _step_dc(layer, x) -> None:
    B = x.shape[0]
    _dc_membrane(layer, x)
    _dc_theta(layer, layer.s)
    if layer.one_spike:
        _one_spike(layer.s.view(B, -1))
    if layer.lbound is not None:
        layer.v.masked_fill_(layer.v < layer.lbound, layer.lbound)
    _trace(layer, layer.s)


def _propagate_mcc(conn, s):
    """MulticompartmentConnection.compute with one Weight (topology.py:437-479, topology_features.py:633-645)."""
    B = s.shape[0]
    spikes = s.reshape(B, conn.source.n, 1).repeat(1, 1, conn.target.n)
    feat = conn._weight()
    signal = feat.value * spikes
    _normalize_step(feat)
    return _sum(signal, 1).view(B, *conn.target.shape)


def _normalize_step(feat) -> None:
    """Weight.compute's closing statement (topology_features.py:641-643): with norm_frequency="time step" the value is normalised in
    place behind the product that read it, at every compute(), learning or not."""
    if feat._norm_step():
        _normalize_columns(feat.value.data, feat.norm, False)


def _propagate_mcc_pipe(conn, s):
    """MulticompartmentConnection.compute with any pipeline of Probability / Mask / Weight / Bias / Intensity: the reference's
    operations in the reference's order (topology.py:437-479; topology_features.py:425-429, :507-508, :633-645, :711-712,
    :755-756), its torch.bernoulli call on the global generator included -- one per Probability and call, whatever the batch."""
    from .topology_features import Bias, Probability, Weight
    conn._check_pipeline()
    B = s.shape[0]
    x = s.reshape(B, conn.source.n, 1).repeat(1, 1, conn.target.n)
    for f in conn.pipeline:
        if isinstance(f, Probability):
            x = x * torch.bernoulli(f.value)
        elif isinstance(f, Weight):
            x = f.value * x
            _normalize_step(f)
        elif isinstance(f, Bias):
            x = x + f.value
        else:                                       # Mask, Intensity
            x = x * f.value
    if tuple(x.shape) != (B, conn.source.n, conn.target.n):
        x = x.view(B, conn.source.n, conn.target.n)
    out = _sum(x, 1) if x.dtype == torch.float32 else x.sum(1)      # (a Mask alone: the reference's integer sum)
    return out.view(B, *conn.target.shape)


def _propagate_conv(conn, s):
    """Conv1d / Conv2d / Conv3dConnection.compute: F.conv1d / conv2d / conv3d (topology.py:640-656, :799-815, :979-995)."""
    conv = (F.conv1d, F.conv2d, F.conv3d)[conn._ndim - 1]
    return conv(s.reshape(s.shape[0], *conn.source.shape).float(), conn.w, conn.b, stride=conn.stride, padding=conn.padding,
                dilation=conn.dilation)


def _propagate_dense(conn, s):
    """Connection / LocalConnection.compute (topology.py:332-346, :1440-1453)."""
    B = s.shape[0]
    post = s.reshape(B, -1).float() @ conn.w.view(conn.source.n, conn.target.n)
    if getattr(conn, "b", None) is not None:
        post = post + conn.b
    return post.view(B, *conn.target.shape)


def _propagate_window(conn, s):
    """Connection.compute_window (topology.py:348-374): the window shifted by one slot, times the current weights."""
    s_w = conn.s_w
    if s_w is None:
        s_w = torch.zeros(conn.target.batch_size, conn.target.res_window_size, *conn.source.shape)
    s_w = torch.cat((s_w[:, 1:, :], s[:, None, :]), 1)
    # (the window is state, not a parameter: written past the `s_w` setter, which would invalidate every network's kept descriptors each step)
    conn.__dict__["_win"] = {"host": s_w, "ring": None, "head": 0}
    if conn.b is None:
        post = s_w.view(s_w.size(0), s_w.size(1), -1).float() @ conn.w
    else:
        post = s_w.view(s_w.size(0), s_w.size(1), -1).float() @ conn.w + conn.b
    return post.view(s_w.size(0), conn.target.res_window_size, *conn.target.shape)


def _propagate_sparse(conn, s):
    """SparseConnection.compute (topology.py:2009-2017 + :332-346): torch's own sparse product, the reference's arithmetic."""
    B = s.shape[0]
    post = s.reshape(B, -1).float() @ conn.w
    if conn.b is not None:
        post = post + conn.b
    return post.view(B, *conn.target.shape)


def _propagate_pool(conn, s):
    """MaxPool1d / 2d / 3dConnection.compute (topology.py:1075-1097 / :1171-1187 / :1261-1277): the rates decay and take the spikes,
    torch's own max_pool picks the indices, the spikes are gathered there."""
    B = s.shape[0]
    fr = conn._rates(B, s.device)
    fr -= conn.decay * fr
    fr += s.float().view(fr.shape)          # (the reference's .squeeze() broadcasts to the same; what it cannot is refused before)
    k, stride, pad, dil = conn._fields()
    pool = getattr(torch.nn.functional, f"max_pool{conn._ndim}d")
    _, idx = pool(fr, kernel_size=k, stride=stride, padding=pad, dilation=dil, return_indices=True)
    return s.reshape(B, fr.shape[1], -1).gather(2, idx.flatten(2)).view_as(idx).float()


def _propagate_avgpool(conn, s):
    """AvgPool2dConnection.compute: torch's own avg_pool2d over the spikes as floats (not in the reference; the device's oracle)."""
    return F.avg_pool2d(s.float().view(s.shape[0], *conn.source.shape), kernel_size=conn.kernel_size, stride=conn.stride, padding=conn.padding,
                        ceil_mode=conn.ceil_mode, count_include_pad=conn.count_include_pad, divisor_override=conn.divisor_override)


def _propagate_permute(conn, s):
    """PermuteConnection.compute (conversion/topology.py:48-56)."""
    return s.permute(conn.dims).float()


def _propagate_pad(conn, s):
    """ConstantPad2dConnection.compute (conversion/topology.py:100-108): F.pad's default fill, 0."""
    return F.pad(s, conn.padding).float()


def _propagate_meanfield(conn, s):
    """MeanFieldConnection.compute (topology.py:1972-1981): the mean over the whole spike tensor, the batch included, times `w`."""
    return s.float().mean() * conn.w


def _update_nothing(conn, kwargs, mask) -> None:
    """SparseConnection, MaxPoolNdConnection, MeanFieldConnection.update: NoOp only (learning.py:87-104 multiplies `w` by 1.0)."""


def _propagate_local(conn, s):
    """LocalConnection1D / 2D / 3D.compute, the reference's expression (topology.py:1573-1597 / :1731-1746 / :1880-1896)."""
    B = s.shape[0]
    s_unfold = conn._unfold(s.reshape(B, *conn.source.shape)).reshape(B, conn.in_channels, conn.conv_prod, conn.kernel_prod)
    a_post = s_unfold.repeat(1, 1, conn.n_filters, 1) * conn.w
    return a_post.sum(-1).sum(1).view(B, *conn.target.shape)


def _update_local(conn, rule) -> None:
    """PostPre on LocalConnection1D / 2D / 3D, the reference's expressions (learning.py:208-389 + :87-104)."""
    B, R, J = conn.source.batch_size, conn.n_filters * conn.conv_prod, conn.in_channels * conn.kernel_prod
    eye = torch.eye(R)

    def unfolded(t):
        u = conn._unfold(t.reshape(B, *conn.source.shape)).reshape(B, conn.conv_prod, J)
        return u.repeat(1, conn.n_filters, 1)

    _postpre_unfolded(conn, rule, conn.target.x.reshape(B, R, 1) * eye, conn.target.s.float().reshape(B, R, 1) * eye, unfolded)


def _postpre_unfolded(conn, rule, target_x, target_s, unfolded) -> None:
    """What the two functions around this one share: one bmm per term against the unfolded source spikes / traces, reduced
    over the batch; then learning.py:87-104 as these families have it (no decay at factor 0, clamp to the connection's bounds)."""
    W = conn.w.data
    if rule.nu[0].any():
        pre = _reduce(rule, torch.bmm(target_x, unfolded(conn.source.s.float())))
        W -= rule.nu[0] * pre.view(W.size())
    if rule.nu[1].any():
        post = _reduce(rule, torch.bmm(target_s, unfolded(conn.source.x)))
        W += rule.nu[1] * post.view(W.size())
    if rule.weight_decay:
        W *= rule.weight_decay
    lo, hi = rule._bounds()
    if lo is not None or hi is not None:
        W.clamp_(conn.wmin, conn.wmax)


def _update_convnd(conn, rule) -> None:
    """PostPre on Conv1dConnection / Conv3dConnection, the reference's expressions (learning.py:422-455 / :499-559 + :87-104).
    The source operands go through the connection's `_pp_unfold`, the reference's own pad + unfold + reshape chain."""
    _lib.raise_if(conn._postpre_error(rule))
    B, Cout = conn.source.batch_size, conn.out_channels
    _postpre_unfolded(conn, rule, conn.target.x.view(B, Cout, -1), conn.target.s.view(B, Cout, -1).float(),
                      lambda t: conn._pp_unfold(t.reshape(B, *conn.source.shape)))


def _reduce(rule, t):
    """`rule.reduction(t, dim=0)` of the per-sample terms [B, ...].  The sums in the serial order this package pins (_sum); mean is that
    sum followed by one true division by B -- the bits of torch.mean on one thread, whose own order follows the caller's thread count;
    amax / amin are exact in any order (the sign of a zero result aside, which torch itself leaves to the path it takes)."""
    if rule.reduction is torch.squeeze:
        return t.squeeze(0)
    if rule.reduction is torch.sum:
        return _sum(t, 0)
    if rule.reduction is torch.mean:
        return _sum(t, 0) / t.shape[0]
    return rule.reduction(t, dim=0)


def _ring_mean(ring):
    """torch.mean(ring, dim=0) of an average_update ring [K, Nin, N] (MCC_learning.py:248, :284, :527, :705): ATen's sum(dim=0) followed
    by one true division by K -- the same bits as torch.mean --, the sum in the serial order this package pins (_sum)."""
    return _sum(ring, 0) / ring.shape[0]


def _mstdp(rule, W, src_s, tgt_s, kwargs) -> None:
    """learning.py:1504-1574 / MCC_learning.py:468-551 (the same arithmetic): the update uses the PREVIOUS step's eligibility
    (kept as its two factors, like on the device: elig[b] = p_plus[b] (x) s_tgt_prev[b] + s_src_prev[b] (x) p_minus[b]),
    then the traces move on.  src_s / tgt_s: [B, n] float spikes of this step."""
    rule._ensure_state()
    reward = kwargs["reward"]
    elig = torch.bmm(rule.p_plus.unsqueeze(2), rule._s_tgt_prev.float().unsqueeze(1)) + \
        torch.bmm(rule._s_src_prev.float().unsqueeze(2), rule.p_minus.unsqueeze(1))
    if isinstance(reward, torch.Tensor) and reward.numel() > 1:
        reward = reward.view(-1, 1, 1).float()
    if getattr(rule, "average_update", 0) > 0:              # MCC_learning.py:518-530
        rule.average_buffer[rule.average_buffer_index] = _reduce(rule, reward * elig)
        rule.average_buffer_index = (rule.average_buffer_index + 1) % rule.average_update
        if rule.continues_update or rule.average_buffer_index == 0:
            W += rule.nu[0] * _ring_mean(rule.average_buffer)
    else:
        W += rule._nu(0) * _reduce(rule, reward * elig)
    _advance_p(rule, *rule._decays(), src_s, tgt_s, kwargs)


def _advance_p(rule, dp, dm, src_s, tgt_s, kwargs) -> None:
    """P+ / P- decay and take this step's spikes, which become the previous step's (learning.py:1560-1570 / :2236-2246)."""
    rule.p_plus *= dp
    rule.p_plus += torch.tensor(kwargs.get("a_plus", 1.0)) * src_s
    rule.p_minus *= dm
    rule.p_minus += torch.tensor(kwargs.get("a_minus", -1.0)) * tgt_s
    rule._s_src_prev, rule._s_tgt_prev = src_s.to(torch.uint8), tgt_s.to(torch.uint8)


def _mstdpet(rule, W, dt, src_s, tgt_s, kwargs) -> None:
    """learning.py:2187-2248 / MCC_learning.py:652-729 (batch 1; src_s / tgt_s flat float spikes): the eligibility TRACE
    takes the previous step's point eligibility, the update is ((nu0 * dt) * reward) * trace, then P+ / P- move on."""
    if rule.source.batch_size != 1:
        raise NotImplementedError("MSTDPET is defined for batch size 1 (learning.py:2211-2212, MCC_learning.py:665-666)")
    rule._ensure_state()
    dp, dm, de = rule._decays()
    rule.eligibility_trace *= de
    rule.eligibility_trace += rule.eligibility / rule.tc_e_trace
    if getattr(rule, "average_update", 0) > 0:              # MCC_learning.py:696-708
        rule.average_buffer[rule.average_buffer_index] = rule.nu[0] * dt * kwargs["reward"] * rule.eligibility_trace
        rule.average_buffer_index = (rule.average_buffer_index + 1) % rule.average_update
        if rule.continues_update or rule.average_buffer_index == 0:
            W += _ring_mean(rule.average_buffer)
    else:
        W += rule.nu[0] * dt * kwargs["reward"] * rule.eligibility_trace
    _advance_p(rule, dp, dm, src_s, tgt_s, kwargs)


def _rmax(rule, W, dt, kwargs) -> None:
    """learning.py:2923-2958 (batch 1), the reference's statements in its order."""
    if rule.source.batch_size != 1:
        raise NotImplementedError(rule._B1)
    rule._reward(kwargs)                               # (a reward the rule does not take raises before anything changes)
    rule._ensure_state()
    target_s = rule.target.s.view(-1).float()
    target_s_prob = rule.target.s_prob.view(-1)
    source_x = rule.source.x.view(-1)
    reward = kwargs["reward"]
    rule.eligibility_trace *= 1 - dt / rule.tc_e_trace
    rule.eligibility_trace += (target_s - (target_s_prob / (1.0 + rule.tc_c / dt * target_s_prob))) * source_x[:, None]
    W += rule.nu[0] * reward * rule.eligibility_trace


def _conv_postpre(conn, rule) -> None:
    """learning.py:457-497: im2col of the source's spikes / traces, one bmm per term, reduced over the batch."""
    from ..utils import im2col_indices
    W = conn.w.data
    Cout, _, kh, kw = W.shape
    B = conn.source.batch_size
    src_x = im2col_indices(conn.source.x.view(B, *conn.source.shape), kh, kw, padding=conn.padding, stride=conn.stride)
    src_s = im2col_indices(conn.source.s.view(B, *conn.source.shape).float(), kh, kw, padding=conn.padding, stride=conn.stride)
    tgt_x, tgt_s = conn.target.x.view(B, Cout, -1), conn.target.s.view(B, Cout, -1).float()
    if rule.nu[0].any():
        W -= rule.nu[0] * _reduce(rule, torch.bmm(tgt_x, src_s.permute(0, 2, 1))).view(W.shape)
    if rule.nu[1].any():
        W += rule.nu[1] * _reduce(rule, torch.bmm(tgt_s, src_x.permute(0, 2, 1))).view(W.shape)


def _conv_mstdp(conn, rule, kwargs) -> None:
    """learning.py:1942-2015 (batch 1).  From its second call on the reference's eligibility has the weight's shape, so its
    torch.sum(update, dim=0) runs over the OUTPUT CHANNELS and is broadcast back (in the first call the eligibility is all
    zeros either way); P+ is kept in input space here -- its im2col goes through the same elementwise operations."""
    from ..utils import im2col_indices
    if conn.source.batch_size != 1:
        raise NotImplementedError("MSTDP on a Conv2dConnection is defined for batch size 1 (learning.py:2013)")
    rule._ensure_state()
    W = conn.w.data
    Cout, _, kh, kw = W.shape
    W += rule.nu[0] * _sum(kwargs["reward"] * rule._elig, 0)
    dp, dm = rule._decays()
    src_s = conn.source.s.view(1, *conn.source.shape).float()
    tgt_s = conn.target.s.view(1, Cout, -1).float()
    rule.p_plus *= dp
    rule.p_plus += torch.tensor(kwargs.get("a_plus", 1.0)) * src_s[0]
    rule.p_minus *= dm
    rule.p_minus += torch.tensor(kwargs.get("a_minus", -1.0)) * tgt_s[0]
    unf = lambda t: im2col_indices(t, kh, kw, padding=conn.padding, stride=conn.stride)      # noqa: E731
    rule._elig = (torch.bmm(tgt_s, unf(rule.p_plus[None]).permute(0, 2, 1)) +
                  torch.bmm(rule.p_minus[None], unf(src_s).permute(0, 2, 1))).view(W.shape)


def _postpre_mcc(rule, W, s_src, x_src, s_tgt, x_tgt, dt) -> None:
    """MCC_learning.py:224-302 + :86-110 on explicit [B, n] factors (parallel.exact_run hands the GLOBAL batch's)."""
    nu0, nu1 = float(rule.nu[0]), float(rule.nu[1])
    K = getattr(rule, "average_update", 0)
    if nu0:
        pre = torch.bmm(s_src.unsqueeze(2).float(), x_tgt.unsqueeze(1) * nu0)
        if K > 0:                                            # MCC_learning.py:237-253: into the ring; its mean when due
            rule.average_buffer_pre[rule.average_buffer_index_pre] = _reduce(rule, pre)
            rule.average_buffer_index_pre = (rule.average_buffer_index_pre + 1) % K
            if rule.continues_update or rule.average_buffer_index_pre == 0:
                W -= _ring_mean(rule.average_buffer_pre) * dt
        else:
            W -= _reduce(rule, pre) * dt
    if nu1:
        post = torch.bmm(x_src.unsqueeze(2), s_tgt.unsqueeze(1).float() * nu1)
        if K > 0:                                            # :273-289
            rule.average_buffer_post[rule.average_buffer_index_post] = _reduce(rule, post)
            rule.average_buffer_index_post = (rule.average_buffer_index_post + 1) % K
            if rule.continues_update or rule.average_buffer_index_post == 0:
                W += _ring_mean(rule.average_buffer_post) * dt
        else:
            W += _reduce(rule, post) * dt
    _decay_clamp(rule, W, rule.decay)


def _update_mcc(conn, dt, kwargs) -> None:
    from ..learning import MCC_learning as rules
    feat = conn._learned()
    if feat is None:                                 # a pipeline without a Weight: nothing learns
        return
    rule = feat.learning_rule
    if isinstance(rule, rules.NoOp) or conn.manual_update:
        return
    B = conn.source.batch_size
    W = feat.value.data
    if not isinstance(rule, rules.MSTDPET):          # (MSTDPET never calls its reduction: MCC_learning.py:652-729)
        from ..learning import _descriptor
        _descriptor.check_reduction(rule)            # (`reduction` may have been assigned since the constructor checked it)
    if rule.reduction is torch.squeeze and B != 1 and not isinstance(rule, rules.MSTDPET):
        raise RuntimeError("reduction=torch.squeeze requires batch size 1")      # (the reference fails with a broadcast error here)
    if isinstance(rule, rules.PostPre):
        _postpre_mcc(rule, W, conn.source.s.view(B, -1), conn.source.x.view(B, -1), conn.target.s.view(B, -1),
                     conn.target.x.view(B, -1), dt)
        return
    if isinstance(rule, rules.MSTDP):
        _mstdp(rule, W, conn.source.s.view(B, -1).float(), conn.target.s.view(B, -1).float(), kwargs)
    elif isinstance(rule, rules.MSTDPET):
        _mstdpet(rule, W, dt, conn.source.s.view(-1).float(), conn.target.s.view(-1).float(), kwargs)
    else:
        raise NotImplementedError(f"bindsnet_amd host path: MCC rule {type(rule).__name__} (supported: PostPre, MSTDP, MSTDPET)")
    _decay_clamp(rule, W, rule.decay)


def _decay_clamp(rule, W, factor) -> None:
    """learning.py:87-104 / MCC_learning.py:86-110: what a rule's update ends with (dense rules keep the factor in
    `weight_decay`, MCC rules in `decay`)."""
    W *= float(factor)
    lo, hi = rule._bounds(tensors=True)
    if isinstance(lo, torch.Tensor) or isinstance(hi, torch.Tensor):       # per-synapse bounds: the reference's own call
        if hasattr(rule, "feature_value"):                                 # MCC_learning.py:110 (a float beside a tensor: as a 0-dim tensor, like the device)
            W.clamp_(*(v if v is None or isinstance(v, torch.Tensor) else torch.tensor(float(v)) for v in (rule.min, rule.max)))
        else:
            W.clamp_(rule.connection.wmin, rule.connection.wmax)           # learning.py:104
    elif lo is not None or hi is not None:
        W.clamp_(lo, hi)


def _update_postpre_only(conn, kwargs, mask) -> None:
    """LocalConnection1D / 2D / 3D and Conv1d / Conv3dConnection.update: PostPre, by the family's `_host_postpre`."""
    rule = conn.update_rule
    if rule._rule_code != _lib.RULE_NONE:
        rule._check_reduction()
        conn._host_postpre(rule)


def _conv_outer_product(conn, rule) -> None:
    """learning.py:1348-1380 (Hebbian) / :920-976 (WeightDependentPostPre): PostPre's two batch-reduced bmm sums, the rule's own statements."""
    from ..learning import learning as rules
    from ..utils import im2col_indices
    W = conn.w.data
    Cout, _, kh, kw = W.shape
    B = conn.source.batch_size
    src_x = im2col_indices(conn.source.x.view(B, *conn.source.shape), kh, kw, padding=conn.padding, stride=conn.stride)
    src_s = im2col_indices(conn.source.s.view(B, *conn.source.shape).float(), kh, kw, padding=conn.padding, stride=conn.stride)
    tgt_x, tgt_s = conn.target.x.view(B, Cout, -1), conn.target.s.view(B, Cout, -1).float()
    pre = lambda: _reduce(rule, torch.bmm(tgt_x, src_s.permute(0, 2, 1))).view(W.shape)       # noqa: E731
    post = lambda: _reduce(rule, torch.bmm(tgt_s, src_x.permute(0, 2, 1))).view(W.shape)      # noqa: E731
    if isinstance(rule, rules.Hebbian):
        W += rule.nu[0] * pre()
        W += rule.nu[1] * post()
        return
    update = 0
    if rule.nu[0].any():
        update -= rule.nu[0] * pre() * (W - conn.wmin)
    if rule.nu[1].any():
        update += rule.nu[1] * post() * (conn.wmax - W)
    W += update


def _update_conv2d(conn, kwargs, mask=None) -> None:
    """Conv2dConnection.update: PostPre, Hebbian, WeightDependentPostPre, MSTDP at batch 1."""
    from ..learning import learning as rules
    rule = conn.update_rule
    if rule is None or isinstance(rule, rules.NoOp):
        return
    if isinstance(rule, rules.PostPre):
        rule._check_reduction()
        _conv_postpre(conn, rule)
    elif isinstance(rule, (rules.Hebbian, rules.WeightDependentPostPre)):
        rule._check_reduction()
        _conv_outer_product(conn, rule)
    elif isinstance(rule, rules.MSTDP):
        _conv_mstdp(conn, rule, kwargs)
    else:
        raise NotImplementedError(f"bindsnet_amd host path: rule {type(rule).__name__} on a Conv2dConnection (supported: PostPre, Hebbian, "
                                  "WeightDependentPostPre, MSTDP)")
    _decay_clamp(rule, conn.w.data, rule.weight_decay)


def _update_dense(conn, kwargs, mask) -> None:
    """Connection / LocalConnection.update: every dense rule on the [source.n, target.n] matrix, then the weight mask."""
    from ..learning import learning as rules
    rule = conn.update_rule
    if rule is None or isinstance(rule, rules.NoOp):
        return
    B = conn.source.batch_size
    W = conn.w.data
    if W.dim() != 2:
        raise NotImplementedError(f"bindsnet_amd host path: rule {type(rule).__name__} on {type(conn).__name__}")
    nu0, nu1 = rule._nu(0), rule._nu(1)                     # floats, or per-synapse tensors (learning.py:67)
    on0 = bool(nu0.any()) if isinstance(nu0, torch.Tensor) else bool(nu0)      # learning.py:399: `self.nu[0].any()`
    on1 = bool(nu1.any()) if isinstance(nu1, torch.Tensor) else bool(nu1)
    if isinstance(rule, rules.MSTDPET):
        _mstdpet(rule, W, conn.dt, conn.source.s.view(-1).float(), conn.target.s.view(-1).float(), kwargs)
    elif isinstance(rule, rules.Rmax):
        _rmax(rule, W, conn.dt, kwargs)
    else:
        rule._check_reduction()
        src_s, tgt_s = conn.source.s.view(B, -1).float(), conn.target.s.view(B, -1).float()
        if isinstance(rule, rules.MSTDP):
            _mstdp(rule, W, src_s, tgt_s, kwargs)
        elif isinstance(rule, (rules.Hebbian, rules.WeightDependentPostPre)):
            # learning.py:1052-1135 / 562-653: raw outer products reduced over the batch, THEN scaled by nu
            u1 = _reduce(rule, torch.bmm(src_s.unsqueeze(2), conn.target.x.view(B, -1).unsqueeze(1)))
            u2 = _reduce(rule, torch.bmm(conn.source.x.view(B, -1).unsqueeze(2), tgt_s.unsqueeze(1)))
            if isinstance(rule, rules.Hebbian):
                W += nu0 * u1
                W += nu1 * u2
            else:
                update = 0
                if on0:
                    update = update - nu0 * u1 * (W - conn.wmin)
                if on1:
                    update = update + nu1 * u2 * (conn.wmax - W)
                W += update
        elif isinstance(rule, rules.PostPre):               # learning.py:390-420
            if on0:
                W -= _reduce(rule, torch.bmm(src_s.unsqueeze(2), conn.target.x.view(B, -1).unsqueeze(1) * nu0))
            if on1:
                W += _reduce(rule, torch.bmm(conn.source.x.view(B, -1).unsqueeze(2), tgt_s.unsqueeze(1) * nu1))
        else:
            raise NotImplementedError(f"bindsnet_amd host path: rule {type(rule).__name__} (supported: PostPre, MSTDP, Hebbian, "
                                      "WeightDependentPostPre, MSTDPET)")
    _decay_clamp(rule, W, rule.weight_decay)
    if mask is not None:
        W.masked_fill_(torch.as_tensor(mask).bool().view_as(W), 0.0)


def run(network, inputs: Dict[str, torch.Tensor], T: int, one_step: bool, kwargs) -> None:
    from .nodes import Input, Nodes
    clamps, unclamps = kwargs.get("clamp", {}) or {}, kwargs.get("unclamp", {}) or {}
    injects_v, masks = kwargs.get("injects_v", {}) or {}, kwargs.get("masks", {}) or {}
    if isinstance(kwargs.get("a_plus"), dict) or isinstance(kwargs.get("a_minus"), dict):
        # network.py:356-378, 432-447 also takes {connection key: value} tables; like the MI355X path (learning/_descriptor.py)
        # this one does not, and says so instead of failing inside torch.tensor(dict)
        raise NotImplementedError("bindsnet_amd: per-connection a_plus/a_minus dicts are not supported")
    for key, conn in network.connections.items():
        if conn._host_refuses_mask and masks.get(key) is not None:
            raise NotImplementedError("bindsnet_amd: weight masks are supported on dense connections")
    for name, layer in network.layers.items():
        if type(layer)._host_step is Nodes._host_step:
            raise NotImplementedError(f"bindsnet_amd host path: layer type {type(layer).__name__}")
        if isinstance(layer, Input) and name not in inputs:
            raise NotImplementedError(f"bindsnet_amd: Input layer '{name}' needs an entry in `inputs`")

    def currents(only=None):
        """Summed input per target layer from the sources' current `s` (network.py:211-250), connection order."""
        cur = {}
        for (src, dst), conn in network.connections.items():
            if only is not None and dst != only:
                continue
            tgt = network.layers[dst]
            window = tgt._gathers_window                 # network.py:232-246: a CSRM layer gathers windows
            if dst not in cur:
                cur[dst] = torch.zeros(network.batch_size, tgt.res_window_size, *tgt.shape) if window else torch.zeros(network.batch_size, *tgt.shape)
            cur[dst] += conn.compute_window(conn.source.s) if window else conn._host_compute(conn.source.s)     # (the connection's own source, as network.py:227)
        return cur

    for t in range(T):
        cur = {} if one_step else currents()
        for name, layer in network.layers.items():
            if isinstance(layer, Input):
                _step_input(layer, inputs[name][t])
            else:
                fed_now = False
                if one_step:
                    own = currents(name)
                    fed_now = name in own
                    cur.update(own)
                x = cur.get(name)
                # an external current for a non-Input layer (network.py:386-392).  With one_step the reference's
                # `current_inputs.update(self._get_inputs(layers=[l]))` (:388-393) REPLACES the entry it has just set for a
                # layer with an incoming connection: the current survives only where no connection feeds the layer
                if name in inputs and not fed_now:
                    ext = inputs[name][t].float()
                    if not (layer._gathers_window and x is not None):     # (a window: `+=` broadcasts the current over its slots, as there)
                        ext = ext.view(network.batch_size, *layer.shape)
                    x = ext.clone() if x is None else x + ext
                if x is None:
                    x = torch.zeros(network.batch_size, *layer.shape)
                inj = injects_v.get(name)
                if inj is not None:
                    inj = torch.as_tensor(inj)
                    layer.v += inj[t] if inj.dim() >= 2 else inj
                layer._host_step(x)
                for table, value in ((clamps, 1), (unclamps, 0)):
                    m = table.get(name)
                    if m is not None:
                        m = clamp_mask(m, layer.n)
                        m = m[t] if m.dim() >= 2 else m
                        layer.s[:, m.view(*layer.shape)] = bool(value)
        if network.learning:
            for key, conn in network.connections.items():
                conn._host_update(kwargs, _mask_of(conn, masks.get(key)))
        for key, conn in network.connections.items():                  # masks apply every step, learning or not
            mask = _mask_of(conn, masks.get(key))
            if mask is not None and hasattr(conn, "w") and conn.w.dim() == 2:
                conn.w.data.masked_fill_(torch.as_tensor(mask).bool().view_as(conn.w), 0.0)
        for m in network.monitors.values():
            m.record()
    if not network.__dict__.get("_defer_norm", False):     # (parallel.sharded_run normalises the MERGED weights itself)
        normalize(network)


def _mask_of(conn, mask):
    """run(..., masks={...}) entry of the connection, else a LocalConnection's structural mask (topology.py:1468-1470)."""
    return mask if mask is not None else getattr(conn, "mask", None)


def _normalize_rows(w, norm) -> None:
    """Every row of the 2-D view `w` scaled to sum `norm`: a Conv2dConnection's [KH*KW] filters (topology.py:824-837), a
    Conv1d / Conv3dConnection's [K] filters (:665-675 / :1004-1017), a LocalConnection1D / 2D / 3D's [kernel_prod] rows
    (:1601 / :1748-1759 / :1898)."""
    for fltr in range(w.shape[0]):
        w[fltr] *= norm / w[fltr].sum(0)


def _normalize_columns(w, norm, use_abs: bool) -> None:
    """Every column of `w` scaled to `norm` -- Weight features by their SIGNED column sums (topology_features.py:250-266), dense
    connections by the absolute ones (topology.py:383-392), a LocalConnection by the signed ones again (topology.py:1475-1482)."""
    colsum = _sum(w.abs() if use_abs else w, 0).unsqueeze(0)
    colsum[colsum == 0] = 1.0
    w *= norm / colsum


def normalize(network) -> None:
    """network.py:463-465: every connection's normalisation."""
    for conn in network.connections.values():
        conn._host_normalize()
