"""The layer-major plan of `Network.run` (`network.layer_major = True`, `last_plan == "layer-major"`): a converted network -- a
feed-forward chain of SubtractiveResetIFNodes without learning -- run layer by layer, each layer over all T steps before the next
one starts, instead of step by step.

Why it is the same run: on the generic plan layer k at step t reads layer k-1's spikes of step t-1 (its `s` at entry for t = 0) and
nothing else, so layer k's whole spike train [T, B, n] follows from layer k-1's whole train.  Per layer, in insertion order:
  * route 1 -- a Conv2dConnection fed spike bytes whose shape `ops.run_conv2d_sif_takes`: ONE launch of snn_run_conv2d_sif_f32, the
    convolution and the IF neurons of all T steps with the neurons' state in registers (csrc/snn_run_conv_sif.hip);
  * route 3 -- a Connection fed spike bytes whose shape passes `_fuse_dense` (what `ops.run_dense_sif_takes`, with or without
    `prop_auto`): ONE launch of snn_run_dense_sif_f32, 16 steps of a sample on the rows of a matrix-core tile and the IF neurons'
    scan along time as the tile's epilogue (csrc/snn_run_dense_sif.hip); no currents scratch;
  * route 2 -- every other connection (AvgPool2dConnection, a Conv2dConnection or Connection its kernel refuses, and a Connection or
    Conv2dConnection fed a real-valued Input): the operator the generic plan calls, called once per time chunk with the chunk's
    frames as Tc x B samples (the frames of a train are contiguous samples; the start frame is a call of its own), into a currents
    scratch, then `ops.sif_scan`, the IF step along time with one thread per neuron.
Every operator is bit-identical to the one the generic plan picks (that is their contract), and both IF kernels call the step's own
bodies, so every train and all state behind the run are the generic plan's, bit for bit; a second run continues exactly.

`prop_stats()` counters are NOT advanced by this plan: which body a tile took per timestep has no meaning here.

A network that asks and does not qualify (`_chain` returns None) runs the generic plan: nothing is raised or printed."""
import torch

from .. import ops
from .monitors import Monitor
from .nodes import Input

# Scratch budget of route 2: the f32 currents [Tc, B, n] of one time chunk.  The chunk length Tc is the largest that fits (at least 1).
CURRENTS_BUDGET_BYTES = 64 << 20
# The most one layer's spike train [T, B, n] may take; a longer run keeps the generic plan.
TRAIN_BUDGET_BYTES = 256 << 20
# Tc * B stays below every operator's batch limit (snn_real.hip and snn_mfma.hip put the sample in a grid dimension: 65535).
MAX_OPERATOR_BATCH = 65535


def _chain(net, req, one_step, kwargs):
    """[(layer name, layer, feeding connection or None)] in insertion order if the graph qualifies, else None."""
    from ..conversion.nodes import SubtractiveResetIFNodes
    from .topology import AvgPool2dConnection, Connection, Conv2dConnection
    d = net.__dict__
    if one_step or kwargs or net.reward_fn is not None or d.get("_pipe") is not None or d.get("_shard_state") is not None \
            or d.get("_defer_norm", False) or req.B > MAX_OPERATOR_BATCH:
        return None
    layers = list(net.layers.items())
    for m in net.monitors.values():                       # spike monitors on layers only: a layer's train IS its raster
        if type(m) is not Monitor or not any(m.obj is l for _, l in layers) or any(v != "s" for v in m.state_vars):
            return None
    feeder, seen, chain = {}, [], []
    for (_, dst), conn in net.connections.items():
        tgt = net.layers.get(dst)
        if type(conn) not in (Connection, Conv2dConnection, AvgPool2dConnection) or tgt is not conn.target or id(tgt) in feeder:
            return None
        if getattr(conn.update_rule, "_learns", False) or conn.norm is not None:
            return None
        w = getattr(conn, "w", None)
        if w is not None and (w.dtype != torch.float32 or not w.is_contiguous()):
            return None
        feeder[id(tgt)] = conn
    for name, layer in layers:
        conn = feeder.get(id(layer))
        if type(layer) is Input:
            if conn is not None or name not in req.inputs or layer.traces:
                return None
        elif type(layer) is SubtractiveResetIFNodes:
            if conn is None or name in req.inputs or not any(conn.source is l for l in seen):
                return None
            if isinstance(conn, AvgPool2dConnection) and conn._batch_refusal(req.B) is not None:
                return None
        else:
            return None
        if req.T * req.B * layer.n > TRAIN_BUDGET_BYTES:
            return None
        seen.append(layer)
        chain.append((name, layer, conn))
    return chain


def _operator(conn, analog: bool, net, dev):
    """The generic plan's operator of `conn` as f(frames [N, *source.shape], out [N, *target.shape])."""
    from .topology import Connection, Conv2dConnection
    if isinstance(conn, Conv2dConnection):
        kw = dict(bias=conn.b.data, stride=conn.stride[0], pad=conn.padding[0])
        if analog:
            return lambda s, out: ops.prop_conv2d_real(conn.w.data, s, out, **kw)
        return lambda s, out: (ops.prop_conv2d_mfma if conn._mfma_route(s.size(0)) else ops.prop_conv2d)(conn.w.data, s, out, **kw)
    if isinstance(conn, Connection):
        W, bias = conn.w.data.view(conn.source.n, conn.target.n), None if conn.b is None else conn.b.data
        if analog:
            return lambda s, out: ops.prop_dense_real(W, s.reshape(s.size(0), -1), out, bias=bias)
        if getattr(conn, "prop_auto", False):
            def dense_auto(s, out):
                flags = net._scratch(("lm_flags", id(conn)), ((s.size(0) + 15) // 16,), torch.int32, dev)
                ops.prop_dense_auto(W, s.reshape(s.size(0), -1), out, bias=bias, flags=flags)
            return dense_auto
        return lambda s, out: ops.prop_dense(W, s.reshape(s.size(0), -1), out, bias=bias)
    return conn._prop_into                                  # AvgPool2dConnection


# Route 3 walks ceil(Nin / 64) slabs per 64 steps whatever N is, about 2.8 us each (profiles/NOTES_layer_major_dense.md): 13 slabs
# (784 sources) is the widest layer measured to win end to end, 128 slabs (8192 -> 10) loses to route 2's one GEMM over T x B samples.
FUSED_DENSE_MAX_SOURCES = 13 * 64


def _fuse_dense(T, B, Nin, N) -> bool:
    """Route 3's gate: whether a Connection fed spike bytes runs as one snn_run_dense_sif_f32 launch."""
    return Nin <= FUSED_DENSE_MAX_SOURCES and ops.run_dense_sif_takes(T, B, Nin, N) != 0


def run(net, req, inputs, one_step, kwargs, dev) -> bool:
    """Run `req` layer-major if the network qualifies (True), else touch nothing (False)."""
    from .topology import Connection, Conv2dConnection
    chain = _chain(net, req, one_step, kwargs)
    if chain is None:
        return False
    T, B = req.T, req.B
    plans = []
    for name, layer, conn in chain:                       # everything that can refuse, before any state changes
        if conn is None:
            x = inputs[name]
            if x.shape[0] < T or x.dtype not in (torch.uint8, torch.bool, torch.float32) or x.numel() != x.shape[0] * B * layer.n:
                return False                              # (the generic plan words the error)
            plans.append(None)
            continue
        pv = {}
        p = layer._params(pv)
        if pv:                                            # per-neuron tc_trace / trace_scale: the generic plan
            return False
        net._check_state(layer, B, dev)
        plans.append((p, layer._summed()))

    trains, starts, analog = {}, {}, {}
    spike_monitors = lambda layer: [m for m in net.monitors.values() if m.obj is layer]      # noqa: E731
    appended = []
    for (name, layer, conn), plan in zip(chain, plans):
        mons = spike_monitors(layer)
        if conn is None:                                  # an Input layer: its train is the caller's tensor
            x = inputs[name].to(dev).contiguous()
            real = name in req.analog
            entry = layer.s
            if real:
                x = x.float()
                if entry.numel() != B * layer.n or entry.device != dev:
                    entry = torch.zeros(B, layer.n, dtype=torch.float32, device=dev)
                entry = entry.float().contiguous()
            elif entry.dtype not in (torch.uint8, torch.bool) or entry.numel() != B * layer.n or entry.device != dev:
                entry = torch.zeros(B, layer.n, dtype=torch.uint8, device=dev)
            inputs[name] = x
            trains[id(layer)], starts[id(layer)], analog[id(layer)] = x[:T], entry.contiguous(), real
            appended += [(m, x[:T].clone().view(T, B, *layer.shape)) for m in mons]
            continue
        p, summed = plan
        src = conn.source
        s_train, s0, real = trains[id(src)], starts[id(src)], analog[id(src)]
        n = layer.n
        if mons:                                          # (new for every call: what an earlier get() handed out is never written again)
            train = torch.empty(T, B, *layer.shape, dtype=torch.bool, device=dev)
        else:
            train = net._scratch(("lm_train", name), (T, B, *layer.shape), torch.bool, dev)
        starts[id(layer)] = layer.s.clone()                # (the layer's `s` is overwritten below; its reader starts from this)
        trains[id(layer)], analog[id(layer)] = train, False
        x = layer.x if layer.traces else None
        geom = None
        if isinstance(conn, Conv2dConnection) and not real:
            geom = (conn.in_channels, src.shape[1], src.shape[2], conn.out_channels, *conn.kernel_size, conn.stride[0], conn.padding[0])
        if geom is not None and ops.run_conv2d_sif_takes(T, B, *geom):
            ops.run_conv2d_sif(conn.w.data, conn.b.data, s0.view(B, *src.shape), s_train if T > 1 else None, train, layer.v,
                               layer.refrac_count, layer.s, p, x=x, summed=summed, stride=conn.stride[0], pad=conn.padding[0])
        elif type(conn) is Connection and not real and _fuse_dense(T, B, src.n, n):
            ops.run_dense_sif(conn.w.data.view(src.n, n), None if conn.b is None else conn.b.data, s0.view(B, src.n),
                              s_train if T > 1 else None, train, layer.v, layer.refrac_count, layer.s, p, x=x, summed=summed)
        else:
            op = _operator(conn, real, net, dev)
            Tc = max(1, min(T, CURRENTS_BUDGET_BYTES // (4 * B * n), MAX_OPERATOR_BATCH // B))
            cur = net._scratch("lm_currents", (Tc * B * n,), torch.float32, dev)
            for t0 in range(0, T, Tc):
                t1 = min(T, t0 + Tc)
                I = cur[:(t1 - t0) * B * n].view(t1 - t0, B, *layer.shape)
                lo = t0
                if t0 == 0:                               # step 0 reads the start frame: a call of its own
                    op(s0.view(B, *src.shape), I[0])
                    lo = 1
                if t1 > lo:                               # steps lo .. t1-1 read frames lo-1 .. t1-2: (t1 - lo) x B contiguous samples
                    op(s_train[lo - 1:t1 - 1].reshape(-1, *src.shape), I[lo - t0:].view(-1, *layer.shape))
                ops.sif_scan(layer.v, layer.refrac_count, layer.s, x, I, train[t0:t1], p, summed=summed)
        appended += [(m, train) for m in mons]

    for name, layer, conn in chain:                       # Input.s aliases the last input slice, as in the reference (nodes.py:219)
        if conn is None:
            layer.s = inputs[name][T - 1]
    for m, buf in appended:
        m._append("s", buf)
    net.__dict__["last_plan"] = "layer-major"
    return True
