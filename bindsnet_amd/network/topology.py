"""Connections: API mirror of bindsnet/network/topology.py for the connection types on the hot
path (`Connection`, `SparseConnection`, `MulticompartmentConnection`, `Conv1dConnection`, `Conv2dConnection`, `Conv3dConnection`,
`LocalConnection`, `LocalConnection1D/2D/3D`, `MaxPool1dConnection`, `MaxPool2dConnection`, `MaxPoo3dConnection`, `MeanFieldConnection`), and `AvgPool2dConnection`, which the reference lacks.  `compute()` launches the
matching propagation kernel of libsnnhip; inside Network.run the same kernels are driven from C++.

`SparseConnection` keeps `w` as a sparse COO Parameter, like the reference, and propagates only: its kernel
(snn_prop_sparse_f32) walks the stored entries of the spiking sources, so its work is spikes x fan-out, and its sums are
bit-identical to the reference's for float weights too.
"""
import warnings
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch.nn import Module, Parameter
from torch.nn.modules.utils import _pair, _triple

from .. import _lib, ops
from .._lib import dptr
from . import host_path
from .nodes import CSRMNodes, Nodes


def _rand_weights(conn, shape, bias_n, w_dtype, kwargs) -> None:
    """`w` and `b` of the convolutional families as the reference draws and clamps them (topology.py:611-630 / :772-791 /
    :950-969): one torch.rand from the global generator, clamped when a bound is infinite, spread over [wmin, wmax] otherwise."""
    w = kwargs.get("w", None)
    inf = torch.tensor(np.inf)
    unbounded = bool((conn.wmin == -inf).any() or (conn.wmax == inf).any())
    if w is None:
        r = torch.rand(*shape)
        w = torch.clamp(r, conn.wmin, conn.wmax) if unbounded else (conn.wmax - conn.wmin) * r + conn.wmin
        w = w.to(dtype=w_dtype)
    else:
        if unbounded:
            w = torch.clamp(w, conn.wmin, conn.wmax)
        w = conn.cast_dtype_if_needed(w, w_dtype)
    conn.w = Parameter(w, requires_grad=False)
    conn.b = Parameter(kwargs.get("b", torch.zeros(bias_n)), requires_grad=False)


def _matrix_weights(conn, w_dtype, kwargs):
    """`w` [source.n, target.n] and the optional `b` of Connection and SparseConnection as the reference draws and clamps them
    (topology.py:309-327)."""
    if w_dtype != torch.float32:
        raise NotImplementedError("bindsnet_amd computes in float32 only")
    w = kwargs.get("w", None)
    unbounded = bool((conn.wmin == -np.inf).any() or (conn.wmax == np.inf).any())
    if w is None:  # consumes the global generator exactly like the reference (topology.py:309-315)
        if unbounded:
            w = torch.clamp(torch.rand(conn.source.n, conn.target.n), conn.wmin, conn.wmax)
        else:
            w = conn.wmin + torch.rand(conn.source.n, conn.target.n) * (conn.wmax - conn.wmin)
        w = w.to(dtype=w_dtype)
    else:
        if bool((conn.wmin != -np.inf).any() or (conn.wmax != np.inf).any()):
            w = torch.clamp(torch.as_tensor(w), conn.wmin, conn.wmax)
        w = conn.cast_dtype_if_needed(w, w_dtype)
    b = kwargs.get("b", None)
    return Parameter(w, requires_grad=False), (Parameter(b, requires_grad=False) if b is not None else None)


def _norm_value(norm):
    """`norm` as ops.normalize takes it: a float, or the tensor of more than one element (one total per target neuron; a
    one-element tensor is a scalar here)."""
    return norm if isinstance(norm, torch.Tensor) and norm.numel() > 1 else float(norm)


def _fill_norm(d, norm, use_abs: int, ws, n: int, dev) -> None:
    """The column-normalisation fields of a snn_conn_desc: a scalar `norm`, or norm_vec for a tensor norm (brought to `dev` once;
    an in-place edit of the tensor rebuilds the kept descriptors)."""
    norm = _norm_value(norm)
    d.has_norm, d.norm_abs, d.norm_ws = 1, use_abs, dptr(ws)
    if isinstance(norm, torch.Tensor):
        vec = ops.norm_vector(norm, n, dev)
        d.norm, d.norm_vec = 0.0, dptr(vec)
    else:
        d.norm = norm


class _Asked:
    """What a run asks of a connection before it starts, for both connection bases; Network.run knows `_refusals` alone."""

    _takes_real = False                # takes a real-valued (float32) source on the device: Connection, Conv2dConnection
    _has_window = False                # has a compute_window that runs in the reference (topology.py:348): Connection

    def _nothing(self, *args):
        return None

    # The pieces, each an exception or None.  _run_refusal(mask, monitored): why no run may start on the connection, given its mask and whether
    # a monitor records it; _learning_refusal(): why no learning run may; _window_refusal(B): why its window cannot take a step at batch size
    # B; _batch_refusal(B): why no run at batch size B may start.  _rule_refusal(rule), asked by LearningRule.__init__: why not this rule.
    _run_refusal = _learning_refusal = _window_refusal = _batch_refusal = _rule_refusal = _nothing

    def _refusals(self, key, req):
        """Why the run `req` must not start with this connection, filed as `key`, in it: exceptions (None: nothing)."""
        yield self._run_refusal(req.masks.get(key), req.monitored(self, key))
        if req.learning:
            yield self._learning_refusal()
        window = self.target._gathers_window
        if window:
            yield self._window_refusal(req.B) if self._has_window else NotImplementedError(
                f"bindsnet_amd: {type(self).__name__} into a CSRMNodes layer is not supported: only Connection has a compute_window "
                "(topology.py:348) that runs in the reference")
        analog = req.analog_source(self) if req.analog else None         # a real-valued input on the device (snnhip.h f17)
        if analog is not None:
            name, x = analog
            if not self._takes_real:
                yield NotImplementedError(f"bindsnet_amd: {type(self).__name__} out of the Input layer '{name}' takes no real-valued "
                                          "(analog) values on the device: its input spike trains must be uint8 or bool "
                                          f"(got {x.dtype}); a float32 input drives Connection and Conv2dConnection only")
            elif self._rule()._learns:
                yield NotImplementedError(f"bindsnet_amd: {type(self._rule()).__name__} on a connection out of the Input layer '{name}' "
                                          "cannot learn from a real-valued (analog) input on the device; use no rule (NoOp)")
            elif window:
                yield NotImplementedError(f"bindsnet_amd: a real-valued (analog) input into the CSRMNodes layer '{key[1]}' is not "
                                          "supported on the device (its window holds spike bytes)")
        yield self._batch_refusal(req.B)

    def _reduction_refusal(self, mode: str, key):
        """parallel.py's modes merge per-shard SUMS of updates: a mean, maximum or minimum over a shard's samples is no part of the global batch's."""
        rule = self._rule()
        reduction = getattr(rule, "reduction", None) if rule._learns else None
        if reduction is not None and reduction is not torch.sum and reduction is not torch.squeeze:
            from ..learning._descriptor import reduction_name
            return NotImplementedError(f"{mode}: {type(self).__name__} {key} has a rule with reduction={reduction_name(reduction)}; the "
                                       "multi-device modes reduce with torch.sum (or torch.squeeze) only; run the network on one device")

    def _multi_device_refusal(self, mode: str, key):
        """The connection's reason against parallel.py's mode `mode`, or None: weights that are no [source.n, target.n] matrices are not routed there."""
        return self._reduction_refusal(mode, key) or (None if self._multi_device else NotImplementedError(
            f"{mode}: {type(self).__name__} {key} is not supported by the multi-device modes; run the network on one device"))


class AbstractConnection(_Asked, _lib.TouchingModule, Module):
    """Reference: topology.py:17-156 (wmin/wmax/norm/update_rule plumbing).

    What a connection family is, is written in its class and asked for by network.py, host_path.py, learning.py and
    parallel.py, none of which names a family: the class-level facts below, `_describe` (its part of a snn_conn_desc),
    `_prop_into` and `_postpre` (its device ops), `_host_compute` / `_host_update` (its host arithmetic in host_path.py).
    The facts default to "nothing": a family that leaves one out is refused, not taken for a dense one."""

    _kind = None                       # snn_conn_desc.kind
    # who normalises: "columns" -- snn_net_run, every column to `norm` (by |w| or signed: _norm_abs) with a [target.n] scratch;
    # "rows" -- snn_net_run, every last-dimension row; "after" -- Network.run calls normalize() behind snn_net_run
    _norm_by = _norm_abs = None
    # run(..., masks=) on the device: refused unless _takes_mask.  The host path refuses only where _host_refuses_mask and
    # ignores the mask on the other families whose `w` is not 2-D: an asymmetry kept as it is
    _takes_mask = _host_refuses_mask = False
    _multi_device = False              # parallel.py's modes refuse it outright (weights gathered through a table)
    # names of the learning.py rules it accepts and, where the refusal comes before anything else in the rule's constructor, its wording
    _rules, _rules_only = frozenset(), None

    def __init__(self, source: Nodes, target: Nodes, nu=None, reduction: Optional[callable] = None,
                 weight_decay: float = 0.0, **kwargs) -> None:
        super().__init__()
        assert isinstance(source, Nodes), "Source is not a Nodes object"
        assert isinstance(target, Nodes), "Target is not a Nodes object"
        self.source, self.target = source, target
        self.weight_decay, self.reduction = weight_decay, reduction
        from ..learning import NoOp
        self.wmin = Parameter(torch.as_tensor(kwargs.get("wmin", -np.inf), dtype=torch.float32), requires_grad=False)
        self.wmax = Parameter(torch.as_tensor(kwargs.get("wmax", np.inf), dtype=torch.float32), requires_grad=False)
        self.norm = kwargs.get("norm", None)
        self.decay = kwargs.get("decay", None)
        if kwargs.get("Dales_rule", None) is not None:
            raise NotImplementedError("bindsnet_amd: Dales_rule is outside the accelerated path")
        self.Dales_rule = None
        rule = kwargs.get("update_rule", None) or NoOp
        self.update_rule = rule(connection=self, nu=nu, reduction=reduction, weight_decay=weight_decay, **kwargs)

    def update(self, **kwargs) -> None:
        """Reference: topology.py:112-139."""
        if kwargs.get("learning", True):
            if not self.w.is_cuda:                        # a connection on the host: plain PyTorch (network/host_path.py)
                self._host_update(kwargs, None)
            else:
                self.update_rule.update(**kwargs)
        mask = kwargs.get("mask", None)
        if mask is not None:                       # topology.py:129-133
            self.w.masked_fill_(torch.as_tensor(mask, device=self.w.device).bool(), 0)

    def compute(self, s: torch.Tensor) -> torch.Tensor:
        """The family's propagation kernel (`_prop_into`) on the device, its host_path function on the host."""
        if not self.w.is_cuda:
            return self._host_compute(s)
        out = torch.empty(s.size(0), *self.target.shape, device=self.w.device)
        self._prop_into(s, out)
        return out

    def normalize(self) -> None:
        """Reference: topology.py:383-392 and its siblings; what is scaled to `norm` is the family's (`_norm_by`)."""
        if self.norm is None:
            return
        if not self.w.is_cuda:
            return self._host_normalize()
        if self._norm_by == "columns":
            ops.normalize(self.w.data.view(self.source.n, self.target.n), _norm_value(self.norm), use_abs=self._norm_abs)
        elif isinstance(self.norm, torch.Tensor):
            raise NotImplementedError("bindsnet_amd: tensor norms are not supported")
        else:                     # every row of the [w.shape[0] * w.shape[1], rest] view (snn_normalize_conv2d)
            ops.normalize_conv2d(self.w.data.view(self.w.shape[0], self.w.shape[1], -1, 1), float(self.norm))

    def _host_normalize(self) -> None:
        if self.norm is not None and self._norm_by != "columns":
            host_path._normalize_rows(self.w.data.view(self.w.shape[0] * self.w.shape[1], -1), self.norm)
        elif self.norm is not None and self.w.dim() == 2:
            host_path._normalize_columns(self.w.data, self.norm, self._norm_abs)

    def _rule(self):
        """The learning rule whose `nu` and descriptor fields belong to this connection."""
        return self.update_rule

    def _weights(self):
        """(owner, attribute) of the learned tensor; the owner also holds its `norm`."""
        return self, "w"

    def _describe(self, d, B: int, dev, scratch) -> list:
        """Fill this connection's part of the snn_conn_desc `d` (d.src / d.dst are set) for batch size B on `dev`; `scratch` is
        Network._scratch.  Returns (owner, attribute) of every tensor whose ADDRESS went in: the descriptor cache re-checks them."""
        if self.w.device != dev:
            raise ValueError("connection weights are not on the network's device; call network.to('cuda')")
        if self.w.dtype != torch.float32 or not self.w.is_contiguous():
            raise NotImplementedError("bindsnet_amd: connection weights must be contiguous float32")
        d.kind, d.w = self._kind, dptr(self.w.data)
        described = [self._weights()]
        if isinstance(getattr(self, "b", None), torch.Tensor):
            d.bias = dptr(self.b.data)
            described.append((self, "b"))
        if self.norm is not None:
            if self._norm_by == "columns":
                ws = scratch(f"norm_{d.src}_{d.dst}", (self.target.n,), torch.float32, dev)
                _fill_norm(d, self.norm, int(self._norm_abs), ws, self.target.n, dev)
            elif isinstance(self.norm, torch.Tensor):
                raise NotImplementedError("bindsnet_amd: tensor norms are not supported")
            elif self._norm_by == "rows":
                d.has_norm, d.norm, d.norm_abs = 1, float(self.norm), 0
        return described

    def _table(self, described: list, name: str, dev):
        """A gather table (an int32 buffer) for `_describe`: its address, once it is on the device and listed in `described`."""
        if getattr(self, name).device != dev:
            raise ValueError("connection tables are not on the network's device; call network.to('cuda')")
        described.append((self, name))
        return dptr(getattr(self, name))

    def _column_slice(self, source: Nodes, target: Nodes, lo: int, hi: int):
        """parallel.column_shard: a connection source -> target holding target columns [lo, hi), same rule and constants (on the host)."""
        raise NotImplementedError(f"column sharding of {type(self).__name__} is not supported")

    def _exact_learns(self) -> bool:
        """parallel.exact_run: whether this connection learns there (a family or rule the mode does not handle raises)."""
        raise NotImplementedError(f"exact_run: connection type {type(self).__name__}")

    def reset_state_variables(self) -> None:
        pass

    @staticmethod
    def cast_dtype_if_needed(w, w_dtype):
        if w.dtype != w_dtype:
            warnings.warn(f"Provided w has data type {w.dtype} but parameter w_dtype is {w_dtype}")
            return w.to(dtype=w_dtype)
        return w


class _FixedConnection(AbstractConnection):
    """The families on which nothing learns and nothing is normalised: NoOp only; a mask, and `norm` where refused, raise `_run_refusal`."""

    _rules = frozenset(("NoOp",))
    _host_update = host_path._update_nothing

    def update(self, **kwargs) -> None:
        if kwargs.get("mask", None) is not None:
            raise self._run_refusal(kwargs["mask"], False)

    def normalize(self) -> None:
        if self.norm is not None:
            _lib.raise_if(self._run_refusal(None, False))

    _host_normalize = normalize


class _DenseConnection(AbstractConnection):
    """What Connection and LocalConnection share: a [source.n, target.n] matrix, propagated by snn_prop_dense_f32, learned by
    every rule of learning.py, its columns normalised."""

    _kind, _norm_by, _norm_abs = _lib.CONN_DENSE, "columns", True
    _takes_mask = _multi_device = True
    _rules = frozenset(("NoOp", "PostPre", "MSTDP", "Hebbian", "WeightDependentPostPre", "MSTDPET", "Rmax"))
    _host_compute, _host_update = host_path._propagate_dense, host_path._update_dense

    def _prop_into(self, s, out, accumulate=False) -> None:
        """s.view(B,-1) @ w (+ b) in canonical ascending-source order (topology.py:332-346).  A float32 `s` on a Connection: the
        same order over real values (ops.prop_dense_real)."""
        if s.dtype == torch.float32 and type(self) is Connection:
            ops.prop_dense_real(self.w.data, s.reshape(s.size(0), -1).contiguous(), out, bias=None if self.b is None else self.b.data,
                                accumulate=accumulate)
            return
        ops.prop_dense(self.w.data, s.reshape(s.size(0), -1).contiguous(), out, bias=None if self.b is None else self.b.data,
                       accumulate=accumulate)

    def _postpre(self, rule, B, lo, hi) -> None:
        """learning.py:390-420."""
        ops.stdp_postpre(self.w.data, self.source.s.reshape(B, -1).contiguous(), self.source.x.reshape(B, -1),
                         self.target.s.reshape(B, -1), self.target.x.reshape(B, -1), rule._nu(0), rule._nu(1),
                         use_dt=False, decay=float(rule.weight_decay), wmin=lo, wmax=hi, reduce=rule._reduce())


class Connection(_DenseConnection):
    """Dense all-to-all synapses (reference: topology.py:265-399)."""

    _takes_real = _has_window = True

    def __init__(self, source: Nodes, target: Nodes, nu=None, reduction=None, weight_decay: float = 0.0,
                 w_dtype: torch.dtype = torch.float32, **kwargs) -> None:
        super().__init__(source, target, nu, reduction, weight_decay, **kwargs)
        self.w, self.b = _matrix_weights(self, w_dtype, kwargs)
        # Not in the reference.  True: on the generic plan the product's body -- matrix cores or event-driven -- is chosen on the device,
        # per tile of 16 samples and timestep, which pays where the source fires densely and costs a second
        # launch per step where it does not; False (the default): the single event-driven launch, as ever.
        self.prop_auto = bool(kwargs.get("prop_auto", False))

    # -- the window of a connection into a CSRMNodes layer (topology.py:329-330, :348-374) ---------------------------------
    # `s_w` reads as the reference's attribute: None until first use, then float32 [B, res_window_size, *source.shape], oldest
    # slot first; it is a plain attribute, not a buffer.  On the device the window is a ring of bytes [B, Wres, source.n] with a
    # head index (snn_prop_window_f32 overwrites the oldest slot); both live in self.__dict__["_win"], which .to() carries along.
    @property
    def s_w(self):
        if not isinstance(self.target, CSRMNodes):
            raise AttributeError(f"'{type(self).__name__}' object has no attribute 's_w'")
        win = self.__dict__.get("_win")
        if win is None:
            return None
        if win["ring"] is None:
            return win["host"]
        ring, head = win["ring"], win["head"]
        return torch.cat((ring[:, head:], ring[:, :head]), 1).float().view(ring.shape[0], ring.shape[1], *self.source.shape)

    @s_w.setter
    def s_w(self, value) -> None:
        self.__dict__["_win"] = None if value is None else {"host": value, "ring": None, "head": 0}
        _lib.touch()

    def _apply(self, fn, *args, **kwargs):
        """nn.Module.to() / cuda() hook: an existing window moves with the weights (the reference leaves it behind)."""
        out = super()._apply(fn, *args, **kwargs)
        if self.w.is_cuda and not self.w.is_contiguous():      # (ann_to_snn's `weight.t()`: same values and shape, row-major for the kernels)
            self.w.data = self.w.data.contiguous()
        win = self.__dict__.get("_win")
        if win is not None:
            for key in ("host", "ring"):
                if win[key] is not None:
                    win[key] = fn(win[key])
        if self.__dict__.get("_prop_counters") is not None:      # (int32: a cast of the module leaves it, a move takes it along)
            self.__dict__["_prop_counters"] = fn(self.__dict__["_prop_counters"])
        return out

    # -- which body the generic plan's propagation took (snn_prop_dense_auto_f32): two int32 words on the device, {matrix, event}
    # tile-steps, added to by the kernels and read only here.  They live in self.__dict__["_prop_counters"], which .to(), clone()
    # and save() carry along.
    def _prop_counter_words(self, dev):
        cnt = self.__dict__.get("_prop_counters")
        if cnt is None:
            cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        self.__dict__["_prop_counters"] = cnt = cnt.to(dev)
        return cnt

    def prop_stats(self) -> dict:
        """{"matrix_tiles", "event_tiles"}: how many (tile of 16 samples, timestep) pairs of Network.run took the matrix-core body and
        how many the event-driven one, since construction or the last reset_prop_stats().  One device read; zeros on the host.  The two
        counters are int32 words: they wrap after 2^31 - 1 tile-steps."""
        cnt = self.__dict__.get("_prop_counters")
        m, e = (0, 0) if cnt is None else cnt.tolist()
        return {"matrix_tiles": int(m), "event_tiles": int(e)}

    def reset_prop_stats(self) -> None:
        if self.__dict__.get("_prop_counters") is not None:
            self.__dict__["_prop_counters"].zero_()

    def _window_ring(self, B: int, dev):
        """The window as snn_prop_window_f32 keeps it, made from `s_w` where that was last written on the host: the "_win" entry
        with a u8 ring [B, Wres, source.n] on `dev`.  A window made for another batch size raises like the reference's cat()."""
        wres = self.target._window_sizes()[0]
        win = self.__dict__.get("_win")
        if win is not None and win["ring"] is not None and win["ring"].device == dev and tuple(win["ring"].shape) == (B, wres, self.source.n):
            return win
        cur = None if win is None else self.s_w
        if cur is None:
            ring = torch.zeros(B, wres, self.source.n, dtype=torch.uint8, device=dev)
        else:
            _lib.raise_if(self._window_refusal(B))
            ring = cur.reshape(B, wres, self.source.n).ne(0).to(dev, torch.uint8).contiguous()
        win = self.__dict__["_win"] = {"host": None, "ring": ring, "head": 0}
        return win

    def _window_refusal(self, B: int):
        """A window made at another batch size or window length: the RuntimeError of the reference's torch.cat (topology.py:359)."""
        win = self.__dict__.get("_win")
        cur = None if win is None else (win["ring"] if win["ring"] is not None else win["host"])
        if cur is None:
            return None
        wres = self.target._window_sizes()[0]
        if cur.shape[0] != B or cur.shape[1] != wres or cur[0, 0].numel() != self.source.n:
            return RuntimeError(f"Sizes of tensors must match except in dimension 1: the window s_w of {type(self).__name__} was made as "
                                f"{[cur.shape[0], cur.shape[1], cur[0, 0].numel()]}, the step needs [{B}, {wres}, {self.source.n}]")
        return None

    def compute_window(self, s: torch.Tensor) -> torch.Tensor:
        """Reference: topology.py:348-374 -- push `s` into the window, return the window times the CURRENT weights (+ b) as
        [B, res_window_size, *target.shape].  On the device snn_prop_window_f32 sums every slot over its spiking sources in
        ascending order."""
        if not self.w.is_cuda:
            return host_path._propagate_window(self, s)
        B = s.size(0)
        win = self._window_ring(B, self.w.device)
        out = torch.empty(B, win["ring"].shape[1], *self.target.shape, device=self.w.device)
        ops.prop_window(self.w.data.view(self.source.n, self.target.n), win["ring"], win["head"], s.reshape(B, -1).contiguous(), out,
                        bias=None if self.b is None else self.b.data)
        win["head"] = (win["head"] + 1) % win["ring"].shape[1]
        return out

    def _describe(self, d, B: int, dev, scratch) -> list:
        if self.w.numel() != self.source.n * self.target.n or (self.b is not None and self.b.numel() != self.target.n):
            # (what torch's matmul / broadcast raises in the first step of the reference; here before the run changes state)
            raise RuntimeError(f"Connection: w {tuple(self.w.shape)} and b {None if self.b is None else tuple(self.b.shape)} do not fit "
                               f"{self.source.n} source and {self.target.n} target neurons")
        described = super()._describe(d, B, dev, scratch)
        if isinstance(self.target, CSRMNodes):
            win = self._window_ring(B, dev)
            d.window, d.win_ring, d.win_head, d.win_size = 1, dptr(win["ring"]), win["head"], win["ring"].shape[1]
        return described

    def _describe_prop(self, p, d, B: int, dev, scratch) -> list:
        """This connection's snn_conn_prop `p` beside its filled snn_conn_desc `d`: spike bytes go through snn_prop_dense_auto_f32 where
        snn_net_run finds the shape worth its second launch (a real-valued Input never reaches it:
        snn_net_run routes that first).  Returns (owner, attribute) pairs like `_describe`."""
        if d.window:
            return []
        flags = scratch(f"prop_flags_{d.src}_{d.dst}", ((B + 15) // 16,), torch.int32, dev)
        p.prop_auto, p.prop_flags, p.prop_counters = int(bool(getattr(self, "prop_auto", False))), dptr(flags), dptr(self._prop_counter_words(dev))
        return [(self, "_prop_counters")]

    def _column_slice(self, source, target, lo, hi):
        def scalar(t) -> float:
            if isinstance(t, torch.Tensor) and t.numel() != 1:
                raise NotImplementedError("column sharding needs scalar wmin / wmax (per-synapse bounds are not supported)")
            return float(t)
        rule = self.update_rule
        from ..learning import MSTDP, PostPre
        rule_cls = type(rule) if isinstance(rule, (PostPre, MSTDP)) else None
        kw = {}
        if isinstance(rule, MSTDP):
            kw.update(tc_plus=float(rule.tc_plus), tc_minus=float(rule.tc_minus))
        return Connection(source, target, w=self.w.data[:, lo:hi].clone().cpu(),
                          b=None if self.b is None else self.b.data[lo:hi].clone().cpu(), wmin=scalar(self.wmin),
                          wmax=scalar(self.wmax), norm=self.norm, update_rule=rule_cls,
                          nu=None if rule_cls is None else (float(rule.nu[0]), float(rule.nu[1])), reduction=rule.reduction,
                          weight_decay=0.0 if rule.weight_decay == 1.0 else 1.0 - float(rule.weight_decay), **kw)

    def _exact_learns(self) -> bool:
        from ..learning import NoOp
        if not isinstance(self.update_rule, NoOp):
            raise NotImplementedError("exact_run: learning on a dense Connection (Input -> Connection -> LIFNodes graphs shard "
                                      "their columns exactly with column_shard, without any collective)")
        return False


class SparseConnection(_FixedConnection):
    """Fixed sparse synapses (reference: topology.py:2009-2017): `Connection`'s constructor, then `w = Parameter(w.to_sparse())`.
    Propagation only.  On the device `compute` is snn_prop_sparse_f32 over a compiled form of `w` (a column-tiled CSR, ops.sparse_compile;
    kept as the non-persistent buffers `sp_ptr` / `sp_col` / `sp_val` and rebuilt when `w` is another tensor, was edited in place or
    has moved); on the host torch's own sparse product.  Both are the reference's arithmetic bit for bit: per column the stored entries
    of the spiking sources in ascending order, then the bias (DESIGN.md "Summation order").

    What the reference does not define on a sparse `w` is refused, where it fails only later in the reference before a run changes
    any state: a learning rule (its update densifies `w`), `norm` (normalize() raises), a `mask` (update()
    raises), Dales_rule, a monitor on `w`, and a `w` that is not float32."""

    _kind = _lib.CONN_SPARSE
    _takes_mask = _multi_device = False
    _rules_only = ("a learning rule adds `update.to_sparse()` to a sparse `w` in the reference, which stores every entry from the "
                   "first step on: that is dense learning, use Connection for it")
    _host_compute = host_path._propagate_sparse

    def __init__(self, source: Nodes, target: Nodes, nu=None, reduction=None, weight_decay: float = 0.0,
                 w_dtype: torch.dtype = torch.float32, **kwargs) -> None:
        super().__init__(source, target, nu, reduction, weight_decay, **kwargs)
        w, self.b = _matrix_weights(self, w_dtype, kwargs)
        self.w = Parameter(w.to_sparse(), requires_grad=False)
        for name in ("sp_ptr", "sp_col", "sp_val"):
            self.register_buffer(name, None, persistent=False)
        self.__dict__["_sp_key"] = None

    def _weights_refusal(self):
        w = self.w
        if not isinstance(w, torch.Tensor) or not w.is_sparse or w.dim() != 2 or tuple(w.shape) != (self.source.n, self.target.n):
            return NotImplementedError(f"bindsnet_amd: SparseConnection.w must be a sparse COO tensor of shape [{self.source.n}, "
                                       f"{self.target.n}]")
        if w.dtype != torch.float32:
            return NotImplementedError(f"bindsnet_amd: SparseConnection.w must be float32 (got {w.dtype}); bindsnet_amd computes in "
                                       "float32 only")
        return None

    def _run_refusal(self, mask, monitored: bool):
        """Why a run must not start on this connection, or None: asked by Network.run before it changes any state."""
        if self.norm is not None:
            return NotImplementedError("SparseConnection with `norm`: the reference's normalize() raises NotImplementedError at the end "
                                       "of the run (aten::eq.Scalar is not defined for a sparse tensor); leave `norm` unset")
        if mask is not None:
            return Exception("Mask isn't supported for SparseConnection")              # topology.py:129-130
        if monitored:
            return NotImplementedError("bindsnet_amd: a monitor on a SparseConnection's `w` is not supported (monitor buffers take "
                                       "the shape of a dense tensor); record connection.w.to_dense() where it is needed")
        return self._weights_refusal()

    def update(self, **kwargs) -> None:
        """Reference: topology.py:112-139 (NoOp leaves `w` as it is; a mask raises)."""
        if kwargs.get("mask", None) is not None:
            raise Exception("Mask isn't supported for SparseConnection")
        if kwargs.get("learning", True):
            self.update_rule.update(**kwargs)

    def _compiled(self):
        """(sp_ptr, sp_col, sp_val) for `w` as it stands.  The key: which tensor `w` is, its in-place version (shared with its
        values and indices), where its values and indices live, and its device."""
        _lib.raise_if(self._weights_refusal())
        w = self.w
        key = (w._version, w._values().data_ptr(), w._indices().data_ptr(), w._nnz(), str(w.device))
        kept = self.__dict__.get("_sp_key")
        if kept is None or kept[0] is not w or kept[1] != key or self.sp_ptr is None or self.sp_ptr.device != w.device:
            self.sp_ptr, self.sp_col, self.sp_val = ops.sparse_compile(w)
            self.__dict__["_sp_key"] = (w, key)
        return self.sp_ptr, self.sp_col, self.sp_val

    def _prop_into(self, s, out, accumulate=False) -> None:
        ops.prop_sparse(self._compiled(), s.reshape(s.size(0), -1).contiguous(), out, bias=None if self.b is None else self.b.data,
                        accumulate=accumulate)

    def _describe(self, d, B, dev, scratch):
        from . import nodes as _nodes
        if self.w.device != dev:
            raise ValueError("connection weights are not on the network's device; call network.to('cuda')")
        _lib.raise_if(self._run_refusal(None, False))
        ptr, col, val = self._compiled()
        d.kind, d.w, d.sparse_nnz = self._kind, None, val.numel()
        d.sparse_ptr, d.sparse_col, d.sparse_val = dptr(ptr), dptr(col), dptr(val)
        if _nodes._SCALARS is not None:                   # an in-place edit of the values moves nothing: the kept descriptors
            _nodes._SCALARS.append((self.w, self.w._version))        # are only good while w's version stands
        described = [(self, "sp_ptr"), (self, "sp_col"), (self, "sp_val")]
        if isinstance(self.b, torch.Tensor):
            if self.b.device != dev or self.b.dtype != torch.float32 or self.b.numel() != self.target.n:
                raise ValueError(f"SparseConnection.b must be a float32 tensor of {self.target.n} entries on the network's device")
            d.bias = dptr(self.b.data)
            described.append((self, "b"))
        return described


class _MaxPoolConnection(_FixedConnection):
    """What MaxPool1dConnection, MaxPool2dConnection and MaxPoo3dConnection (reference: topology.py:1028-1301) share: no weights;
    the state is `firing_rates` [B, *source.shape], an online estimate of every source neuron's rate.  Per `compute(s)` the rates
    decay by `decay` and take the spikes, F.max_poolNd picks every window's highest rate, and the output is the source's spike at
    that position.  On the device one kernel serves the three ranks (snn_prop_pool_f32: the missing dimensions have size 1); on
    the host torch's own max_pool.  Both are the reference's arithmetic bit for bit.

    As the reference, but before a run's first timestep (once its batch size is known): `decay=None` (the default) raises TypeError; a size-1 dimension of
    [B, *source.shape] behind a larger one raises RuntimeError (the reference's `+= s.float().squeeze()` cannot broadcast), and
    so does a target whose shape is not (C, *pooled) or rates kept from another batch size.  Two deliberate deviations: the
    connection runs in training mode (the reference's NoOp multiplies a `w` that does not exist and raises AttributeError), and
    one built before its layers joined a network -- `firing_rates` of shape [0], which raises in the reference until
    reset_state_variables() -- gets zero rates of the right shape at first use.  Masks, monitors and Dales_rule raise."""

    _kind, _ndim, _host_compute = _lib.CONN_POOL, 0, host_path._propagate_pool

    def _init_pool(self, source, target, kwargs) -> None:
        AbstractConnection.__init__(self, source, target, None, None, 0.0, **kwargs)
        self.register_buffer("firing_rates", torch.zeros(source.s.shape))

    def _fields(self):
        """kernel_size, stride, padding, dilation as tuples of `_ndim` ints."""
        nd = self._ndim
        return tuple(tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v),) * nd
                     for v in (self.kernel_size, self.stride, self.padding, self.dilation))

    def _pooled(self):
        """(C, *pooled sizes) of the source's shape; what F.max_poolNd itself refuses raises its RuntimeError here."""
        shape = tuple(self.source.shape)
        if len(shape) != self._ndim + 1:
            raise RuntimeError(f"{type(self).__name__}: the source's shape must be (C, {self._ndim} spatial dimensions), got {shape}")
        k, s, p, d = self._fields()
        fn = getattr(torch.nn.functional, f"max_pool{self._ndim}d")
        key = (shape, k, s, p, d)
        kept = self.__dict__.get("_pooled_kept")         # (kept beside the attributes: it is no state a run descriptor depends on)
        if kept is not None and kept[0] == key:
            return kept[1]
        probe = fn(torch.empty(1, *shape, device="meta"), kernel_size=k, stride=s, padding=p, dilation=d)
        pooled = tuple(probe.shape[1:])
        # A dilated window that misses the plane altogether: torch returns an index outside it.  With torch's own padding <= kernel / 2
        # a window that starts inside the plane has its first tap there, and one that starts in the padding misses only where the
        # plane is narrower than the dilation, which leaves a single window on that axis: the last window decides.
        for a in range(self._ndim):
            start = (pooled[1 + a] - 1) * s[a] - p[a]
            j = -(start // d[a]) if start < 0 else 0            # the first tap at or behind position 0
            if j >= k[a] or start + j * d[a] >= shape[1 + a]:
                raise RuntimeError(f"{type(self).__name__}: the last window of axis {a} has no tap inside the source (F.max_pool"
                                   f"{self._ndim}d returns an index outside the plane there, and the reference's gather raises)")
        self.__dict__["_pooled_kept"] = (key, pooled)
        return pooled

    def _batch_refusal(self, B: int):
        """Why a run at batch size B must not start on this connection, or None: asked by Network.run once the batch size is known."""
        if self.decay is None:
            return TypeError(f"{type(self).__name__} needs `decay=` (the reference multiplies firing_rates by its default, None: "
                             "unsupported operand type(s) for *: 'NoneType' and 'Tensor')")
        full = [int(B), *self.source.shape]
        while full and full[0] == 1:
            full.pop(0)
        if 1 in full:
            return RuntimeError(f"{type(self).__name__}: [batch, *source.shape] = {[int(B), *self.source.shape]} has a size-1 dimension "
                                "behind a larger one; the reference's `firing_rates += s.float().squeeze()` cannot broadcast it")
        try:
            pooled = self._pooled()
        except RuntimeError as e:
            return e
        if tuple(self.target.shape) != pooled:
            return RuntimeError(f"{type(self).__name__}: the target's shape must be {pooled} (channels, then the pooled sizes), got "
                                f"{tuple(self.target.shape)}")
        return None

    def _rates_refusal(self, B: int):
        """Rates kept from another batch size, as in the reference: RuntimeError until reset_state_variables()."""
        fr = self.firing_rates
        if fr.numel() != 0 and tuple(fr.shape) != (int(B), *self.source.shape):
            return RuntimeError(f"{type(self).__name__}: firing_rates has shape {tuple(fr.shape)}, the run needs "
                                f"{(int(B), *self.source.shape)}; call reset_state_variables() after changing the batch size "
                                "(the reference fails the same way)")
        return None

    def _run_refusal(self, mask, monitored: bool):
        if mask is not None:
            return NotImplementedError(f"bindsnet_amd: a mask on a {type(self).__name__} is not supported (it has no weights)")
        if monitored:
            return NotImplementedError(f"bindsnet_amd: a monitor on a {type(self).__name__} (firing_rates) is not supported; read "
                                       "connection.firing_rates after the run")
        return None

    def _refusals(self, key, req):
        yield from super()._refusals(key, req)
        # (a run that CHANGES the batch size meets stale rates where the reference does, in `_rates` behind set_batch_size: DESIGN.md section 1)
        if req.B == self.source.batch_size:
            yield self._rates_refusal(req.B)

    def _rates(self, B: int, dev):
        """`firing_rates` for batch size B on `dev`: zero rates of the right shape where the connection was built before its
        layers joined a network."""
        _lib.raise_if(self._batch_refusal(B) or self._rates_refusal(B))
        if self.firing_rates.numel() == 0:
            self.firing_rates = torch.zeros(int(B), *self.source.shape, device=dev)
        if self.firing_rates.device != torch.device(dev) or self.firing_rates.dtype != torch.float32:
            raise ValueError("firing_rates must be a float32 tensor on the network's device; call network.to('cuda')")
        if not self.firing_rates.is_contiguous():
            self.firing_rates = self.firing_rates.contiguous()
        return self.firing_rates

    def compute(self, s: torch.Tensor) -> torch.Tensor:
        if not s.is_cuda:
            return self._host_compute(s)
        fr = self._rates(s.size(0), s.device)
        out = torch.empty(s.size(0), *self._pooled(), device=s.device)
        self._prop_into(s, out, rates=fr)
        return out

    def _prop_into(self, s, out, accumulate=False, rates=None) -> None:
        fr = self._rates(s.size(0), s.device) if rates is None else rates
        k, st, p, d = self._fields()
        ops.prop_pool(fr, s.reshape(fr.shape).contiguous(), out.view(fr.shape[0], *self._pooled()), k, st, p, d, decay=float(self.decay),
                      accumulate=accumulate)

    def _describe(self, d, B, dev, scratch):
        fr = self._rates(B, dev)
        arrays, _ = ops.pool_geometry(self.source.shape[1:], *self._fields())
        d.kind, d.w, d.firing_rates, d.pool_c, d.pool_decay = self._kind, None, dptr(fr), int(self.source.shape[0]), float(self.decay)
        for name, arr in zip(("pool_in", "pool_k", "pool_stride", "pool_pad", "pool_dil"), arrays):
            for a in range(3):
                getattr(d, name)[a] = arr[a]
        return [(self, "firing_rates")]

    def reset_state_variables(self) -> None:
        """Zero rates for the source's batch size (reference: topology.py:1112-1121)."""
        B = self.source.batch_size
        if B is None:
            return
        if tuple(self.firing_rates.shape) == (B, *self.source.shape):
            self.firing_rates.zero_()
        else:
            self.firing_rates = torch.zeros(B, *self.source.shape, device=self.source.s.device)


class MaxPool1dConnection(_MaxPoolConnection):
    """Max-pooling over a (C, N) source into a (C, L) target (reference: topology.py:1028-1121)."""
    _ndim = 1

    def __init__(self, source: Nodes, target: Nodes, kernel_size: int, stride: int = 1, padding: int = 0, dilation: int = 1,
                 **kwargs) -> None:
        self._init_pool(source, target, kwargs)
        self.kernel_size, self.stride, self.padding, self.dilation = kernel_size, stride, padding, dilation


class MaxPool2dConnection(_MaxPoolConnection):
    """Max-pooling over a (C, H, W) source into a (C, OH, OW) target (reference: topology.py:1124-1211)."""
    _ndim = 2

    def __init__(self, source: Nodes, target: Nodes, kernel_size: Union[int, Tuple[int, int]],
                 stride: Union[int, Tuple[int, int]] = 1, padding: Union[int, Tuple[int, int]] = 0,
                 dilation: Union[int, Tuple[int, int]] = 1, **kwargs) -> None:
        self._init_pool(source, target, kwargs)
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)


class MaxPoo3dConnection(_MaxPoolConnection):
    """Max-pooling over a (C, D, H, W) source into a (C, OD, OH, OW) target (reference: topology.py:1214-1301, where the class
    name lacks its "l"; `MaxPool3dConnection` is the same class)."""
    _ndim = 3

    def __init__(self, source: Nodes, target: Nodes, kernel_size: Union[int, Tuple[int, int, int]],
                 stride: Union[int, Tuple[int, int, int]] = 1, padding: Union[int, Tuple[int, int, int]] = 0,
                 dilation: Union[int, Tuple[int, int, int]] = 1, **kwargs) -> None:
        self._init_pool(source, target, kwargs)
        self.kernel_size, self.stride = _triple(kernel_size), _triple(stride)
        self.padding, self.dilation = _triple(padding), _triple(dilation)


MaxPool3dConnection = MaxPoo3dConnection


class AvgPool2dConnection(_FixedConnection):
    """Average pooling over a (C, H, W) source of 0/1 spikes into a current-driven (C, OH, OW) target: `compute(s)` is
    `F.avg_pool2d(s.float(), kernel_size, stride, padding, ceil_mode, count_include_pad, divisor_override)`, bit for bit.  Not in
    the reference: it is the pooling of a converted CNN (`ann_to_snn` builds it for nn.AvgPool2d and nn.AdaptiveAvgPool2d) -- an
    integrate-and-fire neuron fed count / k^2 fires at the mean rate of its window.  No weights and no state; NoOp only.

    On the device every window is an integer count of spikes, converted to float32 and divided once by the window's divisor
    (snn_prop_avgpool2d_f32, include/snnhip.h f18), so the summation order cannot show; on the host torch's own call.  Window
    placement, the output size with `ceil_mode` and the divisor are ATen's.  `stride=None` is the kernel size, as in torch.

    Before a run changes anything (`_refusals`), each naming the class: a target that is not (C, OH, OW); a PassThroughNodes
    target (its input must be 0 or 1, and an average is a fraction); a real-valued Input source on the device; a mask; a
    monitor; parallel.py's multi-device modes.  `Dales_rule` and `divisor_override=0` raise in the constructor."""

    _kind, _host_compute = _lib.CONN_AVGPOOL, host_path._propagate_avgpool
    _rules_only = "it has no weights, so nothing can learn: use no rule (NoOp)"

    def __init__(self, source: Nodes, target: Nodes, kernel_size: Union[int, Tuple[int, int]],
                 stride: Optional[Union[int, Tuple[int, int]]] = None, padding: Union[int, Tuple[int, int]] = 0, ceil_mode: bool = False,
                 count_include_pad: bool = True, divisor_override: Optional[int] = None, **kwargs) -> None:
        if kwargs.get("Dales_rule", None) is not None:
            raise NotImplementedError("bindsnet_amd: Dales_rule on an AvgPool2dConnection is not supported (it has no weights)")
        if divisor_override is not None and int(divisor_override) == 0:
            raise ValueError("AvgPool2dConnection: divisor_override must not be zero (F.avg_pool2d: divisor must be not zero)")
        AbstractConnection.__init__(self, source, target, kwargs.pop("nu", None), kwargs.pop("reduction", None), kwargs.pop("weight_decay", 0.0),
                                    **kwargs)
        self.kernel_size = _pair(kernel_size)
        self.stride = self.kernel_size if stride is None else _pair(stride)
        self.padding = _pair(padding)
        self.ceil_mode, self.count_include_pad = bool(ceil_mode), bool(count_include_pad)
        self.divisor_override = None if divisor_override is None else int(divisor_override)

    def _pooled(self):
        """(C, OH, OW) of the source's shape; what F.avg_pool2d itself refuses (a pad beyond half the kernel, an empty output) raises
        its RuntimeError here."""
        shape = tuple(self.source.shape)
        if len(shape) != 3:
            raise RuntimeError(f"AvgPool2dConnection: the source's shape must be (C, H, W), got {shape}")
        key = (shape, self.kernel_size, self.stride, self.padding, self.ceil_mode)
        kept = self.__dict__.get("_pooled_kept")         # (kept beside the attributes, as _MaxPoolConnection keeps its own)
        if kept is not None and kept[0] == key:
            return kept[1]
        probe = torch.nn.functional.avg_pool2d(torch.empty(1, *shape, device="meta"), kernel_size=self.kernel_size, stride=self.stride,
                                               padding=self.padding, ceil_mode=self.ceil_mode)
        pooled = tuple(probe.shape[1:])
        self.__dict__["_pooled_kept"] = (key, pooled)
        return pooled

    def _batch_refusal(self, B: int):
        from ..conversion.nodes import PassThroughNodes
        if isinstance(self.target, PassThroughNodes):
            return NotImplementedError("bindsnet_amd: AvgPool2dConnection into a PassThroughNodes layer is not supported: that layer's "
                                       "input must be 0 or 1, and an average over a window is a fraction; use a current-driven layer "
                                       "(SubtractiveResetIFNodes, IFNodes, ...)")
        try:
            pooled = self._pooled()
        except RuntimeError as e:
            return RuntimeError(f"AvgPool2dConnection: {e}") if "AvgPool2dConnection" not in str(e) else e
        if tuple(self.target.shape) != pooled:
            return RuntimeError(f"AvgPool2dConnection: the target's shape must be {pooled} (channels, then the pooled sizes), got "
                                f"{tuple(self.target.shape)}")
        return None

    def _run_refusal(self, mask, monitored: bool):
        if mask is not None:
            return NotImplementedError("bindsnet_amd: a mask on an AvgPool2dConnection is not supported (it has no weights)")
        if monitored:
            return NotImplementedError("bindsnet_amd: a monitor on an AvgPool2dConnection is not supported (it has no state)")
        return None

    def _args(self) -> dict:
        return dict(kernel_size=self.kernel_size, stride=self.stride, padding=self.padding, ceil_mode=self.ceil_mode,
                    count_include_pad=self.count_include_pad, divisor_override=self.divisor_override)

    def compute(self, s: torch.Tensor) -> torch.Tensor:
        if not s.is_cuda:
            return self._host_compute(s)
        out = torch.empty(s.size(0), *self._pooled(), device=s.device)
        self._prop_into(s, out)
        return out

    def _prop_into(self, s, out, accumulate=False) -> None:
        _lib.raise_if(self._batch_refusal(s.size(0)))
        if s.dtype not in (torch.bool, torch.uint8):
            raise NotImplementedError(f"bindsnet_amd: AvgPool2dConnection takes 0/1 spikes (bool or uint8) on the device, got {s.dtype}")
        B = s.size(0)
        ops.prop_avgpool(s.reshape(B, *self.source.shape).contiguous(), out.view(B, *self._pooled()), accumulate=accumulate, **self._args())

    def _describe(self, d, B, dev, scratch):
        _lib.raise_if(self._batch_refusal(B))
        arrays, _ = ops.avgpool_geometry(self.source.shape[1:], self.kernel_size, self.stride, self.padding, self.ceil_mode)
        d.kind, d.w, d.avgp_c = self._kind, None, int(self.source.shape[0])
        for name, arr in zip(("avgp_in", "avgp_k", "avgp_stride", "avgp_pad"), arrays):
            for a in range(2):
                getattr(d, name)[a] = arr[a]
        d.avgp_ceil, d.avgp_include_pad = int(self.ceil_mode), int(self.count_include_pad)
        d.avgp_divisor = 0 if self.divisor_override is None else self.divisor_override
        return []


class MeanFieldConnection(_FixedConnection):
    """Mean-field synapses (reference: topology.py:1920-2006): `compute(s) = s.float().mean() * w`, the mean over the whole
    [B, *source.shape] tensor, the batch included.  `w` is 0-dim (the default: one randn draw) or a tensor that broadcasts onto
    [B, *target.shape]; a recurrent connection with a negative scalar `w` is global inhibition.  On the device the spikes are
    counted as integers and the mean is f32(count) / f32(numel), which is the reference's mean up to 2^24 elements
    (snn_prop_meanfield_f32); on the host the reference's expression.  Propagation only, in training and eval mode.

    As the reference: the constructor hands `weight_decay` on in the `reduction` slot, so it never reaches the rule; a given `w`
    is clamped only when a bound is infinite; a rule other than NoOp raises NotImplementedError at construction.  `norm=` raises
    NotImplementedError before a run changes any state (the reference's normalize() raises TypeError behind the run: it assigns
    a plain tensor to the Parameter `w`).  Masks, monitors, Dales_rule, a `w` that is not float32 and batch x source.n beyond
    2^24 raise."""

    _kind, _host_compute = _lib.CONN_MEANFIELD, host_path._propagate_meanfield

    def __init__(self, source: Nodes, target: Nodes, nu=None, weight_decay: float = 0.0, w_dtype: torch.dtype = torch.float32,
                 **kwargs) -> None:
        super().__init__(source, target, nu, weight_decay, **kwargs)          # (sic: topology.py:1957)
        if w_dtype != torch.float32:
            raise NotImplementedError("bindsnet_amd computes in float32 only")
        w = kwargs.get("w", None)
        unbounded = bool((self.wmin == -np.inf).any() or (self.wmax == np.inf).any())
        if w is None:
            r = (torch.randn(1)[0] + 1) / 10
            w = torch.clamp(r, self.wmin, self.wmax) if unbounded else self.wmin + r * (self.wmax - self.wmin)
            w = w.to(dtype=w_dtype)
        else:
            if unbounded:
                w = torch.clamp(w, self.wmin, self.wmax)
            w = self.cast_dtype_if_needed(w, w_dtype)
        self.w = Parameter(w, requires_grad=False)

    def _w_refusal(self, B: int):
        w = self.w
        if not isinstance(w, torch.Tensor) or w.dtype != torch.float32:
            return NotImplementedError(f"bindsnet_amd: MeanFieldConnection.w must be float32 (got {getattr(w, 'dtype', type(w))}); "
                                       "bindsnet_amd computes in float32 only")
        full = (int(B), *self.target.shape)
        shape = tuple(w.shape)
        while shape and shape[0] == 1:
            shape = shape[1:]
        if len(shape) > len(full) or shape != full[len(full) - len(shape):]:
            return NotImplementedError(f"bindsnet_amd: MeanFieldConnection.w must have one element or the shape of a tail of "
                                       f"[batch, *target.shape] = {list(full)}; got {list(w.shape)}")
        return None

    def _batch_refusal(self, B: int):
        if int(B) * self.source.n > _lib.MEANFIELD_MAX:
            return NotImplementedError(f"bindsnet_amd: MeanFieldConnection over batch x source.n = {int(B) * self.source.n} elements is "
                                       "not supported (f32(count) / f32(numel) is the reference's mean up to 2^24 elements)")
        return self._w_refusal(B)

    def _run_refusal(self, mask, monitored: bool):
        if self.norm is not None:
            return NotImplementedError("MeanFieldConnection with `norm`: the reference's normalize() raises TypeError at the end of the "
                                       "run (it assigns a plain tensor to the Parameter `w`); leave `norm` unset")
        if mask is not None:
            return NotImplementedError("bindsnet_amd: a mask on a MeanFieldConnection is not supported")
        if monitored:
            return NotImplementedError("bindsnet_amd: a monitor on a MeanFieldConnection is not supported (nothing changes `w`)")
        return None

    def compute(self, s: torch.Tensor) -> torch.Tensor:
        """A tensor of w's shape, as in the reference (Network.run broadcasts it onto the target)."""
        if not self.w.is_cuda:
            return self._host_compute(s)
        _lib.raise_if(self._batch_refusal(s.size(0)))
        out = torch.empty_like(self.w.data)
        ops.prop_meanfield(self.w.data.contiguous(), s.reshape(1, -1).contiguous(), out.view(1, -1), store=True)
        return out

    def _prop_into(self, s, out, accumulate=False) -> None:
        _lib.raise_if(self._batch_refusal(s.size(0)))
        ops.prop_meanfield(self.w.data.contiguous(), s.reshape(s.size(0), -1).contiguous(), out.view(s.size(0), -1), accumulate=accumulate)

    def _describe(self, d, B, dev, scratch):
        if self.w.device != dev:
            raise ValueError("connection weights are not on the network's device; call network.to('cuda')")
        _lib.raise_if(self._run_refusal(None, False) or self._batch_refusal(B))
        if not self.w.is_contiguous():
            raise NotImplementedError("bindsnet_amd: connection weights must be contiguous float32")
        d.kind, d.w, d.w_numel = self._kind, dptr(self.w.data), self.w.numel()
        return [(self, "w")]


class LocalConnection(_DenseConnection):
    """Locally connected synapses (reference: topology.py:1304-1485): a dense [source.n, target.n] matrix that is zero
    outside each target neuron's receptive field (`mask`), propagated like `Connection` (+ bias), learned with the dense
    rules, masked again after every update, normalised by the SIGNED column sums (norm scaled by the kernel size).  Like
    the reference it draws its initial weights from numpy's global generator, and its `compute` output carries no batch
    dimension, i.e. it is meant for batch size 1."""

    _norm_abs = False                  # signed column sums (topology.py:1475-1482)

    def __init__(self, source: Nodes, target: Nodes, kernel_size: Union[int, Tuple[int, int]],
                 stride: Union[int, Tuple[int, int]], n_filters: int, nu=None, reduction=None, weight_decay: float = 0.0,
                 w_dtype: torch.dtype = torch.float32, **kwargs) -> None:
        super().__init__(source, target, nu, reduction, weight_decay, **kwargs)
        if w_dtype != torch.float32:
            raise NotImplementedError("bindsnet_amd computes in float32 only")
        self.kernel_size, self.stride, self.n_filters = _pair(kernel_size), _pair(stride), n_filters
        shape = kwargs.get("input_shape", None)
        if shape is None:
            shape = _pair(int(np.sqrt(source.n)))
        kh, kw = self.kernel_size
        if self.kernel_size == tuple(shape):
            conv_size = [1, 1]
        else:
            conv_size = (int((shape[0] - kh) / self.stride[0]) + 1, int((shape[1] - kw) / self.stride[1]) + 1)
        self.conv_size = conv_size
        conv_prod, kernel_prod = int(np.prod(conv_size)), int(np.prod(self.kernel_size))
        assert target.n == n_filters * conv_prod, (
            f"Total neurons in target layer must be {n_filters * conv_prod}. Got {target.n}.")
        # source index of tap (k1, k2) of receptive field (c1, c2) -- with the reference's own row stride for k1
        # (shape[0], topology.py:1420-1427)
        c1, c2 = torch.arange(conv_size[0]).view(1, 1, -1, 1), torch.arange(conv_size[1]).view(1, 1, 1, -1)
        k1, k2 = torch.arange(kh).view(-1, 1, 1, 1), torch.arange(kw).view(1, -1, 1, 1)
        locations = (c1 * self.stride[0] * shape[1] + c2 * self.stride[1] + k1 * shape[0] + k2).long()
        self.register_buffer("locations", locations.reshape(kernel_prod, conv_prod))
        w = kwargs.get("w", None)
        unbounded = bool((self.wmin == -np.inf).any() or (self.wmax == np.inf).any())
        if w is None:
            w = torch.zeros(source.n, target.n)
            for f in range(n_filters):                       # same visiting order as the reference: the draws come
                for c in range(conv_prod):                   # from numpy's global generator one at a time
                    for k in range(kernel_prod):
                        w[self.locations[k, c], f * conv_prod + c] = np.random.rand()
            w = torch.clamp(w, self.wmin, self.wmax) if unbounded else self.wmin + w * (self.wmax - self.wmin)
            w = w.to(dtype=w_dtype)
        else:
            if not unbounded or bool((self.wmin != -np.inf).any() or (self.wmax != np.inf).any()):
                w = torch.clamp(torch.as_tensor(w), self.wmin, self.wmax)
            w = self.cast_dtype_if_needed(w, w_dtype)
        self.w = Parameter(w, requires_grad=False)
        self.register_buffer("mask", self.w == 0)
        self.b = Parameter(kwargs.get("b", torch.zeros(target.n)), requires_grad=False)
        if self.norm is not None:
            self.norm *= kernel_prod

    def compute(self, s: torch.Tensor) -> torch.Tensor:
        out = super().compute(s)
        return out.view(*self.target.shape) if s.size(0) == 1 else out

    def update(self, **kwargs) -> None:
        if kwargs.get("mask", None) is None:
            kwargs["mask"] = self.mask
        super().update(**kwargs)


class Conv2dConnection(AbstractConnection):
    """2-D convolutional synapses (reference: topology.py:686-844): propagation, PostPre, Hebbian, WeightDependentPostPre, and MSTDP
    at batch 1.  MSTDPET is not offered: the reference's conv2d form (learning.py:2654-2745) never adds the point eligibility to its
    eligibility trace, so it leaves the weights as they are at batch 1 and fails at larger batches.

    Propagation takes any number of input channels.  On the device every output is the sequential f32 sum over (kh, kw, cin), input
    channels innermost, bias last: up to 16 channels that is the reference's own order; beyond, the reference's oneDNN order depends
    on the host, and the device equals it bit for bit where every partial sum is exact, else up to summation rounding (INTEGRATION.md
    section 3).  The host path calls F.conv2d itself.  The learning rules stop at 16 input channels (`_rule_refusal`)."""

    _kind, _ndim = _lib.CONN_CONV2D, 2
    _norm_by = "after"      # every [KH*KW] filter to sum `norm` (topology.py:824-837): not snn_net_run's column step
    _multi_device = _takes_real = True
    _rules = frozenset(("NoOp", "PostPre", "Hebbian", "WeightDependentPostPre", "MSTDP"))
    _rules_only = "PostPre, Hebbian, WeightDependentPostPre and MSTDP are"      # (any other rule: named in LearningRule's error)
    _outer_product_rules = (_lib.RULE_POSTPRE, _lib.RULE_HEBBIAN, _lib.RULE_WDPOSTPRE)
    _host_compute, _host_update = host_path._propagate_conv, host_path._update_conv2d

    def __init__(self, source: Nodes, target: Nodes, kernel_size: Union[int, Tuple[int, int]],
                 stride: Union[int, Tuple[int, int]] = 1, padding: Union[int, Tuple[int, int]] = 0,
                 dilation: Union[int, Tuple[int, int]] = 1, nu=None, reduction=None, weight_decay: float = 0.0,
                 w_dtype: torch.dtype = torch.float32, **kwargs) -> None:
        super().__init__(source, target, nu, reduction, weight_decay, **kwargs)
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)
        if self.dilation != (1, 1) or self.stride[0] != self.stride[1] or self.padding[0] != self.padding[1]:
            raise NotImplementedError("bindsnet_amd: conv2d supports dilation 1 and symmetric stride/padding only")
        self.in_channels, ih, iw = source.shape[0], source.shape[1], source.shape[2]
        self.out_channels = target.shape[0]
        oh = int((ih - self.kernel_size[0] + 2 * self.padding[0]) / self.stride[0] + 1)
        ow = int((iw - self.kernel_size[1] + 2 * self.padding[1]) / self.stride[1] + 1)
        assert target.shape[1] == oh and target.shape[2] == ow, (
            "Target dimensionality must be (out_channels, ?,"
            "(input_height - filter_height + 2 * padding_height) / stride_height + 1,"
            "(input_width - filter_width + 2 * padding_width) / stride_width + 1")
        _rand_weights(self, (self.out_channels, self.in_channels, *self.kernel_size), self.out_channels, w_dtype, kwargs)

    def _rule_refusal(self, rule):
        """Why `rule` must not be constructed on this connection, or None: asked by LearningRule.__init__ (the connection's own
        constructor has not run yet, so the channel count is the source's)."""
        cin = self.source.shape[0]
        if cin > 16 and rule._learns:
            return NotImplementedError(
                f"bindsnet_amd: {type(rule).__name__} on a Conv2dConnection with {cin} input channels is not supported: the "
                f"reference reduces the update with torch.bmm over an operand in_channels * KH * KW wide, whose summation "
                f"order has not been characterised beyond 16 input channels (propagation runs at any width; use NoOp or no rule)")
        return None

    def _prop_into(self, s, out, accumulate=False) -> None:
        if s.dtype == torch.float32:                   # real-valued sources: the same tap order (ops.prop_conv2d_real)
            ops.prop_conv2d_real(self.w.data, s.reshape(s.size(0), *self.source.shape).contiguous(), out, bias=self.b.data,
                                 stride=self.stride[0], pad=self.padding[0], accumulate=accumulate)
            return
        ops.prop_conv2d(self.w.data, s.contiguous(), out, bias=self.b.data, stride=self.stride[0], pad=self.padding[0],
                        accumulate=accumulate)

    def _describe(self, d, B, dev, scratch):
        if self.b.numel() != self.out_channels:       # (F.conv2d's RuntimeError in the first step of the reference; here before the run changes state)
            raise RuntimeError(f"Conv2dConnection: the bias has {self.b.numel()} entries, the convolution {self.out_channels} output channels")
        described = super()._describe(d, B, dev, scratch)
        d.cin, d.h, d.wd = self.in_channels, self.source.shape[1], self.source.shape[2]
        d.cout, d.kh, d.kw = self.out_channels, self.kernel_size[0], self.kernel_size[1]
        d.stride, d.pad = self.stride[0], self.padding[0]
        if getattr(self.update_rule, "_rule_code", None) in self._outer_product_rules:      # learning.py:457-497, :920-976, :1348-1380: per-sample partial sums live in scratch
            d.rule_ws = dptr(scratch(f"convpp_{d.src}_{d.dst}", (2 * B * self.w.numel(),), torch.float32, dev))
        return described

    def _postpre(self, rule, B, lo, hi) -> None:
        """learning.py:457-497."""
        src, tgt = self.source, self.target
        ops.conv2d_postpre(self.w.data, src.s.reshape(B, *src.shape).contiguous(), src.x.reshape(B, *src.shape),
                           tgt.s.reshape(B, *tgt.shape), tgt.x.reshape(B, *tgt.shape), float(rule.nu[0]), float(rule.nu[1]),
                           stride=self.stride[0], pad=self.padding[0], decay=float(rule.weight_decay), wmin=lo, wmax=hi, reduce=rule._reduce())

    def _outer_product(self, rule, B, lo, hi) -> None:
        """learning.py:1348-1380 (Hebbian) / :920-976 (WeightDependentPostPre)."""
        src, tgt = self.source, self.target
        ops.conv2d_hebbian(self.w.data, src.s.reshape(B, *src.shape).contiguous(), src.x.reshape(B, *src.shape),
                           tgt.s.reshape(B, *tgt.shape), tgt.x.reshape(B, *tgt.shape), float(rule.nu[0]), float(rule.nu[1]),
                           weight_dependent=rule._weight_dependent, stride=self.stride[0], pad=self.padding[0],
                           decay=float(rule.weight_decay), wmin=lo, wmax=hi, reduce=rule._reduce())


class _ConvNdConnection(AbstractConnection):
    """What Conv1dConnection and Conv3dConnection (reference: topology.py:540-683, :847-1025) share.  Weights [Cout, Cin,
    *kernel], bias `b` zeros(Cout).  `compute` runs snn_prop_convnd_f32 on the device (one kernel for both: a conv1d is the
    conv3d with D = H = 1), the reference's F.conv1d / F.conv3d on the host.

    PostPre (learning.py:422-455 / :499-559) hands torch.bmm a source operand built by pad + unfold + a raw reshape; that
    matrix is kept as the int32 buffer `pp_src` [L, Cin*K]: the reference's own expressions (`_pp_unfold`) applied to
    arange(source.n) + 1, so that 0 marks padding (stored as -1).  It reproduces conv1d's raw view (which mixes channels and
    positions when Cin > 1) and conv3d's swapped unfold axes without restating them.  When those expressions fail, or give
    another L than the target's position count (the reference's bmm then fails), the table is empty and PostPre raises."""

    _kind, _ndim = _lib.CONN_CONVND, 0
    _norm_by = "after"      # every [K] filter of the [Cout*Cin, K] view to sum `norm` (topology.py:665-675 / :1004-1017)
    _host_refuses_mask = True
    _rules, _rules_only = frozenset(("NoOp", "PostPre")), "PostPre is"
    _host_compute, _host_update, _host_postpre = host_path._propagate_conv, host_path._update_postpre_only, host_path._update_convnd

    def _init_weights(self, shape, w_dtype, kwargs) -> None:
        """The weights, and the PostPre gather table `pp_src`."""
        _rand_weights(self, shape, self.out_channels, w_dtype, kwargs)
        J = self.in_channels * int(np.prod(self._kernel()))
        self._pp_error = None
        try:
            idx = (torch.arange(self.source.n, dtype=torch.int64) + 1).view(1, *self.source.shape)
            tab = self._pp_unfold(idx)[0] - 1
            if tab.shape[0] != int(np.prod(self.target.shape[1:])):
                raise RuntimeError(f"the unfolded source has {tab.shape[0]} positions, the target "
                                   f"{int(np.prod(self.target.shape[1:]))}")
        except RuntimeError as e:
            self._pp_error = (f"PostPre on this {type(self).__name__} fails in the reference (its torch.bmm operands do not "
                              f"match: {e})")
            tab = torch.empty(0, J, dtype=torch.int64)
        self.register_buffer("pp_src", tab.to(torch.int32).contiguous())

    def _kernel(self):
        return (self.kernel_size,) if self._ndim == 1 else self.kernel_size

    def _stride(self):
        return self.stride if self._ndim == 1 else self.stride[0]        # (isotropic: checked by Conv3dConnection's constructor)

    def _padding(self):
        return self.padding if self._ndim == 1 else self.padding[0]

    def _postpre_error(self, rule):
        """Why the reference's PostPre update fails on this connection (a RuntimeError), or None."""
        if self._ndim == 3 and bool(rule.nu[0] != 0):
            # learning.py:526-547: source_s is never cast to float, so torch.bmm(target_x, source_s) raises
            return RuntimeError("PostPre on a Conv3dConnection with nu[0] != 0 fails in the reference: torch.bmm raises 'expected m1 and m2 "
                                "to have the same dtype, but got: float != bool' (learning.py:526-551, source_s is never cast to float); "
                                "use nu[0] == 0 or network.train(False)")
        return None if self._pp_error is None else RuntimeError(self._pp_error)

    def _learning_refusal(self):
        # PostPre on a Conv3dConnection with nu[0] != 0 fails in the reference at its first learning step (a bool bmm
        # operand); here before the run changes any state -- a deliberate deviation in timing
        return self._postpre_error(self.update_rule) if self.update_rule._rule_code == _lib.RULE_POSTPRE else None

    def _prop_into(self, s, out, accumulate=False) -> None:
        ops.prop_convnd(self.w.data, s.reshape(s.size(0), *self.source.shape).contiguous(), out, bias=self.b.data,
                        stride=self._stride(), pad=self._padding(), accumulate=accumulate)

    def _describe(self, d, B, dev, scratch):
        described = super()._describe(d, B, dev, scratch)
        k = self._kernel()
        d.cin, d.cout = self.in_channels, self.out_channels
        d.conv_nd, d.stride, d.pad = self._ndim, self._stride(), self._padding()
        unit = (1,) * (3 - self._ndim)                        # a conv1d is the conv3d with D = H = 1
        (d.conv_d, d.h, d.wd), (d.conv_kd, d.kh, d.kw) = unit + tuple(self.source.shape[1:]), unit + tuple(k)
        d.conv_pp_src, d.conv_pp_rows = self._table(described, "pp_src", dev), self.pp_src.shape[0]
        if getattr(self.update_rule, "_rule_code", None) == _lib.RULE_POSTPRE:      # the packed target spikes, when they exceed the kernel's LDS
            L = max(int(self.pp_src.shape[0]), 1)
            d.rule_ws = dptr(scratch(f"convndpp_{d.src}_{d.dst}", (B * self.out_channels * ((L + 31) // 32),), torch.int32, dev))
        return described

    def _postpre(self, rule, B, lo, hi) -> None:
        """learning.py:422-455 / :499-559."""
        _lib.raise_if(self._postpre_error(rule))
        src, tgt = self.source, self.target
        ops.convnd_postpre(self.w.data, self.pp_src, src.s.reshape(B, -1).contiguous(), src.x.reshape(B, -1),
                           tgt.s.reshape(B, -1).contiguous(), tgt.x.reshape(B, -1), float(rule.nu[0]), float(rule.nu[1]),
                           decay=float(rule.weight_decay), wmin=lo, wmax=hi, reduce=rule._reduce())


class Conv1dConnection(_ConvNdConnection):
    """1-D convolutional synapses, source shape (Cin, N), target (Cout, L) (reference: topology.py:540-683): propagation and
    PostPre.  Input channels are limited to 16 (the reference's oneDNN accumulation order is characterised up to there)."""

    _ndim = 1

    def __init__(self, source: Nodes, target: Nodes, kernel_size: int, stride: int = 1, padding: int = 0, dilation: int = 1,
                 nu=None, reduction=None, weight_decay: float = 0.0, w_dtype: torch.dtype = torch.float32, **kwargs) -> None:
        super().__init__(source, target, nu, reduction, weight_decay, **kwargs)
        if dilation != 1:
            raise NotImplementedError("Dilation is not currently supported for 1-D spiking convolution.")
        self.kernel_size, self.stride, self.padding, self.dilation = kernel_size, stride, padding, dilation
        self.in_channels, input_size = source.shape[0], source.shape[1]
        self.out_channels, output_size = target.shape[0], target.shape[1]
        conv_size = (input_size - self.kernel_size + 2 * self.padding) / self.stride + 1
        assert target.shape[0] == self.out_channels and target.shape[1] == int(conv_size), (
            "Target dimensionality must be (out_channels, ?,(input_size - filter_size + 2 * padding) / stride + 1,")
        if self.in_channels > 16:
            raise NotImplementedError("bindsnet_amd: Conv1dConnection with more than 16 input channels is not supported (the "
                                      "reference's oneDNN accumulation order is only characterised up to 16)")
        if self.in_channels > 1 and self.kernel_size == 1:
            raise NotImplementedError("bindsnet_amd: Conv1dConnection with kernel_size 1 and more than one input channel is not "
                                      "supported (the reference's oneDNN takes a 1x1 kernel whose order depends on the shape)")
        self._init_weights((self.out_channels, self.in_channels, self.kernel_size), w_dtype, kwargs)

    def _pp_unfold(self, t: torch.Tensor) -> torch.Tensor:
        """learning.py:434-438 on t [B, Cin, N]."""
        t = torch.nn.functional.pad(t, _pair(self.padding))
        return t.unfold(-1, self.kernel_size, self.stride).reshape(t.shape[0], -1, self.in_channels * self.kernel_size)


class Conv3dConnection(_ConvNdConnection):
    """3-D convolutional synapses, source shape (Cin, D, H, W), target (Cout, OD, OH, OW) (reference: topology.py:847-1025):
    propagation and PostPre with nu[0] == 0.  One input channel (the reference's oneDNN order at Cin > 1 depends on the
    shape), isotropic stride and padding.

    Deviation: PostPre with nu[0] != 0 fails in the reference at the first learning step, after that step's neuron update
    (learning.py:526-551 hands torch.bmm a bool operand).  Here Network.run raises the same RuntimeError before the run
    changes any state."""

    _ndim = 3

    def __init__(self, source: Nodes, target: Nodes, kernel_size: Union[int, Tuple[int, int, int]],
                 stride: Union[int, Tuple[int, int, int]] = 1, padding: Union[int, Tuple[int, int, int]] = 0,
                 dilation: Union[int, Tuple[int, int, int]] = 1, nu=None, reduction=None, weight_decay: float = 0.0,
                 w_dtype: torch.dtype = torch.float32, **kwargs) -> None:
        super().__init__(source, target, nu, reduction, weight_decay, **kwargs)
        if dilation != 1 and dilation != (1, 1, 1):
            raise NotImplementedError("Dilation is not currently supported for 3-D spiking convolution.")
        self.kernel_size, self.stride = _triple(kernel_size), _triple(stride)
        self.padding, self.dilation = _triple(padding), _triple(dilation)
        self.in_channels, idepth, iheight, iwidth = source.shape[0], source.shape[1], source.shape[2], source.shape[3]
        self.out_channels = target.shape[0]
        out = [int((n - k + 2 * p) / s + 1) for n, k, p, s in zip((idepth, iheight, iwidth), self.kernel_size, self.padding,
                                                                  self.stride)]
        assert target.shape[0] == self.out_channels and list(target.shape[1:4]) == out, (
            "Target dimensionality must be (out_channels, ?,"
            "(input_depth - filter_depth + 2 * padding_depth) / stride_depth + 1,"
            "(input_height - filter_height + 2 * padding_height) / stride_height + 1,"
            "(input_width - filter_width + 2 * padding_width) / stride_width + 1")
        if self.in_channels != 1:
            raise NotImplementedError("bindsnet_amd: Conv3dConnection supports one input channel (the reference's oneDNN "
                                      "accumulation order at Cin > 1 depends on the shape)")
        if len(set(self.stride)) != 1 or len(set(self.padding)) != 1:
            raise NotImplementedError("bindsnet_amd: Conv3dConnection supports isotropic stride and padding only")
        if self.padding[0] and any(n == 1 and k == 1 for n, k in zip((idepth, iheight), self.kernel_size[:2])):
            raise NotImplementedError("bindsnet_amd: Conv3dConnection with padding and a depth or height of 1 with a kernel of 1 "
                                      "is not supported (the kernel's C ABI reads such an axis as unpadded)")
        self._init_weights((self.out_channels, self.in_channels, *self.kernel_size), w_dtype, kwargs)

    def _pp_unfold(self, t: torch.Tensor) -> torch.Tensor:
        """learning.py:523-534 on t [B, Cin, D, H, W] (D unfolded with the kernel's width, W with its depth, as there)."""
        kd, kh, kw = self.kernel_size
        p, s = self.padding, self.stride
        t = torch.nn.functional.pad(t, (p[0], p[0], p[1], p[1], p[2], p[2]))
        return t.unfold(-3, kw, s[0]).unfold(-3, kh, s[1]).unfold(-3, kd, s[2]).reshape(t.shape[0], -1,
                                                                                           self.in_channels * kw * kh * kd)


class _LocalConnectionND(AbstractConnection):
    """What LocalConnection1D / 2D / 3D (reference: topology.py:1488-1910) share.  Weights [Cin, n_filters*conv_prod,
    kernel_prod]; target neuron r = f*conv_prod + o sees receptive field o.  The three classes differ only in the `unfold`
    calls that gather a receptive field's source spikes, so the gather is kept as a table: the int32 buffer `src`
    [Cin, conv_prod, kernel_prod] holds the flat source index of every tap, built by pushing arange(source.n) through
    those same unfolds (`_unfold`).  `compute` and PostPre (learning.py:208-389) run in libsnnhip (snn_prop_local_f32,
    snn_local_postpre); on the host the reference's own torch expressions (network/host_path.py).

    Deviation: the reference's `w=` branch asserts against an attribute it never defines (`self.out_channels`) and so
    raises AttributeError for any `w`; here a `w` of shape [Cin, n_filters*conv_prod, kernel_prod] is accepted (and clamped
    to [wmin, wmax] like a drawn one), any other shape raises AssertionError."""

    _kind, _ndim = _lib.CONN_LOCAL, 0
    _norm_by = "rows"       # every [kernel_prod] row to sum `norm` (topology.py:1748-1759): snn_net_run, through snn_normalize_conv2d
    _rules, _rules_only = frozenset(("NoOp", "PostPre")), "PostPre is"
    _host_compute, _host_update, _host_postpre = host_path._propagate_local, host_path._update_postpre_only, host_path._update_local

    def __init__(self, source: Nodes, target: Nodes, kernel_size, stride, n_filters: int, nu=None, reduction=None,
                 weight_decay: float = 0.0, w_dtype: torch.dtype = torch.float32, **kwargs) -> None:
        super().__init__(source, target, nu, reduction, weight_decay, **kwargs)
        if w_dtype != torch.float32:
            raise NotImplementedError("bindsnet_amd computes in float32 only")
        nd = self._ndim
        self.n_filters = n_filters
        self.in_channels = source.shape[0]
        spatial = [int(v) for v in source.shape[1:1 + nd]]
        ks = kernel_size if nd == 1 else tuple(kernel_size)
        st = stride if nd == 1 else tuple(stride)
        kl, sl = ([ks], [st]) if nd == 1 else (list(ks), list(st))
        conv = [int((spatial[i] - kl[i]) / sl[i]) + 1 for i in range(nd)]
        self.conv_size = conv[0] if nd == 1 else tuple(conv)
        self.conv_prod, self.kernel_prod = int(np.prod(conv)), int(np.prod(kl))
        idx = torch.arange(self.in_channels * int(np.prod(spatial))).view(1, self.in_channels, *spatial)
        self.register_buffer("src", self._unfold(idx).reshape(self.in_channels, self.conv_prod, self.kernel_prod)
                             .to(torch.int32).contiguous())
        shape = (self.in_channels, self.n_filters * self.conv_prod, self.kernel_prod)
        w = kwargs.get("w", None)
        if w is None:            # topology.py:1551-1554 / :1704-1707 / :1853-1856: one draw from the global generator
            w = torch.rand(*shape).to(dtype=w_dtype)
        else:
            assert tuple(w.shape) == shape, ("Target dimensionality must be (in_channels,n_filters*conv_prod,kernel_prod)")
            w = self.cast_dtype_if_needed(w, w_dtype)
        if self.wmin != -np.inf or self.wmax != np.inf:
            w = torch.clamp(w, self.wmin, self.wmax)
        self.w = Parameter(w, requires_grad=False)
        self.b = Parameter(kwargs.get("b", None), requires_grad=False)

    def _unfold(self, t: torch.Tensor) -> torch.Tensor:
        """The reference's unfold chain on t [B, Cin, *spatial] -> [B, Cin, conv..., kernel...] (a view)."""
        if self._ndim == 1:
            return t.unfold(-1, self.kernel_size, self.stride)
        for i in range(self._ndim):
            t = t.unfold(-self._ndim, self.kernel_size[i], self.stride[i])
        return t

    def _prop_into(self, s, out, accumulate=False) -> None:
        """a_post = unfold(s) * w; a_post.sum(-1).sum(1) (topology.py:1573-1597 / :1731-1746 / :1880-1896)."""
        ops.prop_local(self.w.data, self.src, s.reshape(s.shape[0], -1).contiguous(), out, self.n_filters, accumulate=accumulate)

    def _describe(self, d, B, dev, scratch):
        described = super()._describe(d, B, dev, scratch)
        d.bias, d.cin, d.local_src = None, self.in_channels, self._table(described, "src", dev)
        d.local_F, d.local_conv_prod, d.local_kernel_prod, d.local_n_src = self.n_filters, self.conv_prod, self.kernel_prod, self.source.n
        return described

    def _postpre(self, rule, B, lo, hi) -> None:
        """learning.py:208-389."""
        src, tgt = self.source, self.target
        ops.local_postpre(self.w.data, self.src, src.s.reshape(B, -1).contiguous(), src.x.reshape(B, -1),
                          tgt.s.reshape(B, -1).contiguous(), tgt.x.reshape(B, -1), float(rule.nu[0]), float(rule.nu[1]),
                          self.n_filters, decay=float(rule.weight_decay), wmin=lo, wmax=hi, reduce=rule._reduce())

    def reset_state_variables(self) -> None:
        super().reset_state_variables()
        self.target.reset_state_variables()          # as the reference does (topology.py:1612-1618)


class LocalConnection1D(_LocalConnectionND):
    """One-dimensional local connection, source shape (C, H) (reference: topology.py:1488-1618)."""
    _ndim = 1

    def __init__(self, source: Nodes, target: Nodes, kernel_size: int, stride: int, n_filters: int, nu=None, reduction=None,
                 weight_decay: float = 0.0, w_dtype: torch.dtype = torch.float32, **kwargs) -> None:
        self.kernel_size, self.stride = kernel_size, stride
        super().__init__(source, target, kernel_size, stride, n_filters, nu, reduction, weight_decay, w_dtype, **kwargs)


class LocalConnection2D(_LocalConnectionND):
    """Two-dimensional local connection, source shape (C, H, W) (reference: topology.py:1621-1767)."""
    _ndim = 2

    def __init__(self, source: Nodes, target: Nodes, kernel_size: Union[int, Tuple[int, int]], stride: Union[int, Tuple[int, int]],
                 n_filters: int, nu=None, reduction=None, weight_decay: float = 0.0, w_dtype: torch.dtype = torch.float32,
                 **kwargs) -> None:
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        super().__init__(source, target, self.kernel_size, self.stride, n_filters, nu, reduction, weight_decay, w_dtype, **kwargs)


class LocalConnection3D(_LocalConnectionND):
    """Three-dimensional local connection, source shape (C, H, W, D) (reference: topology.py:1770-1917)."""
    _ndim = 3

    def __init__(self, source: Nodes, target: Nodes, kernel_size: Union[int, Tuple[int, int, int]],
                 stride: Union[int, Tuple[int, int, int]], n_filters: int, nu=None, reduction=None, weight_decay: float = 0.0,
                 w_dtype: torch.dtype = torch.float32, **kwargs) -> None:
        self.kernel_size, self.stride = _triple(kernel_size), _triple(stride)
        super().__init__(source, target, self.kernel_size, self.stride, n_filters, nu, reduction, weight_decay, w_dtype, **kwargs)


class AbstractMulticompartmentConnection(_Asked, _lib.TouchingModule, Module):
    """Reference: topology.py:159-262 (feature pipeline bookkeeping)."""

    def __init__(self, source: Nodes, target: Nodes, device, pipeline: list = None, **kwargs) -> None:
        super().__init__()
        assert isinstance(source, Nodes), "Source is not a Nodes object"
        assert isinstance(target, Nodes), "Target is not a Nodes object"
        self.source, self.target, self.device = source, target, device
        self.pipeline = [] if pipeline is None else pipeline
        self.feature_index = {}
        for feature in self.pipeline:
            self.feature_index[feature.name] = feature
            feature.prime_feature(connection=self, device=self.device, **kwargs)

    def append_pipeline(self, feature) -> None:
        self.pipeline.append(feature)
        feature.prime_feature(connection=self, device=self.device)
        self.feature_index[feature.name] = feature

    def remove_pipeline(self, feature) -> None:
        self.pipeline.remove(feature)
        del self.feature_index[feature.name]

    def _apply(self, fn, *a, **k):
        """nn.Module.to()/cuda() hook: also move feature values, which live in a plain python list
        and which the reference leaves behind on the CPU (SURVEY.md finding 8)."""
        out = super()._apply(fn, *a, **k)
        probe = fn(torch.empty(0))
        for f in self.pipeline:
            f.to(probe.device)
        self.device = probe.device
        return out


class MulticompartmentConnection(AbstractMulticompartmentConnection):
    """Feature-pipeline connection (reference: topology.py:402-537).  A pipeline of exactly one `Weight` is
    snn_prop_cascade_f32; every other ordered pipeline of up to 8 features out of Probability / Mask / Weight / Bias /
    Intensity is a feature program evaluated per synapse (snn_mcc_bernoulli + snn_prop_mcc_pipe_f32 on the device,
    host_path._propagate_mcc_pipe on the host).  The single Weight may be float16 or bfloat16 (DiehlAndCook2015(w_dtype=...)):
    snn_prop_cascade_h16 / snn_stdp_postpre_h16 / snn_normalize_h16 with the reference's roundings (csrc/snn_half.hpp), NoOp or
    PostPre only; plain torch on the host."""

    _kind = _lib.CONN_MCC
    _norm_by = "columns"               # the Weight's SIGNED column sums (topology_features.py:250-266), by snn_net_run
    _takes_mask = _host_refuses_mask = False           # (no `w`: the device path refuses a mask, the host path ignores it)
    _MAX_PIPE = 8                      # SNN_MCC_MAX_PIPE
    # How a single Weight with norm_frequency="time step" is propagated and normalised (snn_conn_desc.norm_step): 1 -- snn_prop_cascade_f32
    # and snn_normalize(_pv), 2 -- snn_prop_cascade_norm(_pv)_f32, one launch.  The two forms leave the same bits; the three launches are
    # the faster ones at the flagship shape (profiles/NOTES_norm_step.md: the fused kernel keeps 25 workgroups busy, k_prop 64), so they
    # are what runs.  tools/bench_norm_step.py and tests/test_gpu_norm_step.py select the other form through this attribute.
    _NORM_STEP_FORM = 1

    def __init__(self, source: Nodes, target: Nodes, device, pipeline: list = [], manual_update: bool = False,
                 traces: bool = False, **kwargs) -> None:
        super().__init__(source, target, device, pipeline, **kwargs)
        self.traces, self.manual_update = traces, manual_update
        if traces:
            # topology.py:434-435, :473-474: the connection's own [B, target.n] contribution of the last step, "for monitors".  On
            # the device a float32 buffer that Network.run's propagation writes (snn_conn_desc.activity), on the host the sum itself
            self.activity = None

    def _names(self) -> list:
        return [type(f).__name__ for f in self.pipeline]

    def _single(self) -> bool:
        """The pipeline of exactly one Weight: today's code path and descriptor."""
        from .topology_features import Weight
        return len(self.pipeline) == 1 and isinstance(self.pipeline[0], Weight)

    @property
    def _multi_device(self) -> bool:
        return self._single()

    def _multi_device_refusal(self, mode, key):
        half = self._half_dtype()
        if half is not None:               # the modes merge, slice and gather float32 matrices
            return NotImplementedError(f"{mode}: MulticompartmentConnection {key} has a {half} Weight; the multi-device modes compute in "
                                       "float32 only; run the network on one device")
        if any(getattr(f.learning_rule, "average_update", 0) for f in self.pipeline):
            # an averaging ring is one history of the GLOBAL batch's updates: a shard's own ring, or a slice of one, is another rule
            return NotImplementedError(f"{mode}: MulticompartmentConnection {key} has a rule with average_update, whose ring of past updates "
                                       "the multi-device modes neither merge nor slice; run the network on one device")
        if any(getattr(f, "norm_frequency", "sample") == "time step" for f in self.pipeline):
            # every step normalises the GLOBAL matrix's columns before that step's update: a merge of shard deltas after the run cannot
            return NotImplementedError(f"{mode}: MulticompartmentConnection {key} has a Weight with norm_frequency='time step', which the "
                                       "multi-device modes do not reproduce; run the network on one device")
        err = self._reduction_refusal(mode, key)
        if err is None and self.traces:
            # `activity` is the step's sum over the GLOBAL source layer and batch: a column or batch shard's own is another tensor
            return NotImplementedError(f"{mode}: MulticompartmentConnection {key} has traces=True, whose `activity` the multi-device modes "
                                       "neither merge nor slice; run the network on one device")
        return err or (None if self._single() else NotImplementedError(
            f"{mode}: MulticompartmentConnection {key} with the feature pipeline {self._names()} is not supported by the multi-device modes "
            "(a single Weight is); run the network on one device"))

    def _check_pipeline(self) -> None:
        from .topology_features import Bias, Intensity, Mask, Probability, Weight
        if not self.pipeline or len(self.pipeline) > self._MAX_PIPE or \
                any(type(f) not in (Probability, Mask, Weight, Bias, Intensity) for f in self.pipeline):
            raise NotImplementedError(f"bindsnet_amd runs MulticompartmentConnection pipelines of 1 to {self._MAX_PIPE} features out of "
                                      f"Probability, Mask, Weight, Bias, Intensity; got {self._names()}")

    def _learned(self):
        """The Weight the rule, the norm and the weight monitors refer to: the one with a learning rule if there is one, else
        the only one; None for a pipeline without a Weight (or with several and no rule)."""
        from ..learning.MCC_learning import NoOp
        from .topology_features import Weight
        self._check_pipeline()
        ws = [f for f in self.pipeline if isinstance(f, Weight)]
        ruled = [f for f in ws if not isinstance(f.learning_rule, NoOp) and f.learning_rule is not None]
        if len(ruled) > 1:
            raise NotImplementedError(f"bindsnet_amd: at most one Weight of a pipeline may have a learning rule; got {self._names()}")
        if ruled:
            return ruled[0]
        return ws[0] if len(ws) == 1 else None

    def _weight(self):
        feat = self._learned()
        if feat is None:
            raise NotImplementedError(f"bindsnet_amd: the pipeline {self._names()} has no single Weight to refer to")
        return feat

    def _single_weight(self, what: str):
        if not self._single():
            raise NotImplementedError(f"{what}: MulticompartmentConnection with the feature pipeline {self._names()} is not supported "
                                      "(a single Weight is)")
        return self.pipeline[0]

    def _half_dtype(self):
        """torch.float16 / torch.bfloat16 if a feature's value has that dtype, else None."""
        for f in self.pipeline:
            if isinstance(f.value, torch.Tensor) and f.value.dtype in ops.HALF:
                return f.value.dtype
        return None

    def _run_refusal(self, mask, monitored: bool):
        """What a float16 / bfloat16 Weight cannot run, asked by Network.run before anything changes: it is supported as the single
        feature of the pipeline, without a rule or with PostPre, unmonitored."""
        half = self._half_dtype()
        if half is None:
            return None
        from ..learning import MCC_learning
        if monitored:
            return NotImplementedError(f"bindsnet_amd: a Monitor on a MulticompartmentConnection with a {half} Weight is not supported")
        if self._single():
            feat = self.pipeline[0]
            if isinstance(feat.learning_rule, (MCC_learning.MSTDP, MCC_learning.MSTDPET)):
                return NotImplementedError(f"bindsnet_amd: MCC {type(feat.learning_rule).__name__} on a {half} Weight is not supported "
                                           "(NoOp and PostPre are)")
            if isinstance(feat.norm, torch.Tensor):
                return NotImplementedError(f"bindsnet_amd: tensor norms are not supported on a {half} Weight")
        if any(getattr(f, "norm_frequency", "sample") == "time step" for f in self.pipeline):
            return NotImplementedError(f"bindsnet_amd: norm_frequency='time step' on a {half} Weight is not supported (float32 is)")
        return None

    def _on_host(self) -> bool:
        return bool(self.pipeline) and all(isinstance(f.value, torch.Tensor) and not f.value.is_cuda for f in self.pipeline)

    def _float_result(self) -> bool:
        """Whether the reference's pipeline result is float32 (what the device computes): some feature's value is."""
        return any(isinstance(f.value, torch.Tensor) and f.value.dtype == torch.float32 for f in self.pipeline)

    def compute(self, s: torch.Tensor) -> torch.Tensor:
        """out[b,j] = sum_i term(b,i,j) in the reference's ATen sum order (topology.py:437-479)."""
        B = s.size(0)
        self._check_pipeline()
        if self._on_host():
            return self._host_compute(s)
        dev = self.pipeline[0].value.device
        out = torch.empty(B, self.target.n, device=dev)
        self._prop_into(s.reshape(B, -1).contiguous(), out)
        half = self._half_dtype() if self._single() else None
        if self.traces:
            self.activity = out
        if half is not None:                    # the reference returns the sum in the Weight's dtype; the values already are
            out = out.to(half)
        return out.view(B, *self.target.shape)

    def _host_compute(self, s):
        out = host_path._propagate_mcc(self, s) if self._single() else host_path._propagate_mcc_pipe(self, s)
        if self.traces:
            self.activity = out.reshape(s.shape[0], self.target.n)
        return out

    def _activity_buffer(self, d, B, dev) -> list:
        """traces=True on the device: `activity` as the float32 [B, target.n] buffer the run's propagation writes and a Monitor's
        record segment reads.  Returns the (owner, attribute) pair whose address `d` now holds."""
        if not self.traces:
            return []
        act = self.__dict__.get("activity")
        if not isinstance(act, torch.Tensor) or tuple(act.shape) != (B, self.target.n) or act.dtype != torch.float32 \
                or act.device != dev or not act.is_contiguous():
            self.activity = torch.zeros(B, self.target.n, device=dev)
        d.activity = dptr(self.activity)
        return [(self, "activity")]

    def _program(self, dev, scratch, key):
        """The feature program of a multi-feature pipeline on `dev`: [(kind, value tensor, scalar flag, bit workspace)] in
        pipeline order, and the features whose values' addresses it holds."""
        from .topology_features import Bias, Mask, Probability, Weight
        self._check_pipeline()
        S, N = self.source.n, self.target.n
        if not self._float_result():
            raise NotImplementedError(f"bindsnet_amd: the pipeline {self._names()} does not yield float32 in the reference; it runs on "
                                      "the host path only")
        prog = []
        for k, f in enumerate(self.pipeline):
            if f.value.device != dev:
                f.to(dev)
            val = f.value
            want = torch.bool if isinstance(f, Mask) else torch.float32
            if val.dtype != want or not val.is_contiguous() or (tuple(val.shape) != (S, N) and val.numel() != 1):
                raise NotImplementedError(f"bindsnet_amd: {type(f).__name__}.value must be a contiguous {want} [{S}, {N}] tensor or a "
                                          f"single element (got {val.dtype}, shape {tuple(val.shape)})")
            kind = _lib.MCC_OP_MUL_DRAW if isinstance(f, Probability) else _lib.MCC_OP_MUL_MASK if isinstance(f, Mask) else \
                _lib.MCC_OP_ADD_F32 if isinstance(f, Bias) else _lib.MCC_OP_MUL_F32
            bits = scratch(f"mccbits_{key}_{k}", (S * ((N + 31) // 32),), torch.int32, dev) if kind == _lib.MCC_OP_MUL_DRAW else None
            prog.append((kind, f, int(val.numel() == 1), bits))
        return prog

    def _prop_into(self, s, out, accumulate=False) -> None:
        if self._single():
            feat = self.pipeline[0]
            if feat._norm_step() and self._NORM_STEP_FORM == 2:
                return ops.prop_cascade_norm(feat.value.data, s, out, _norm_value(feat.norm), accumulate=accumulate)
            ops.prop_cascade(feat.value.data, s, out, accumulate=accumulate)
            if feat._norm_step():                  # Weight.compute normalises behind its product (topology_features.py:641-643)
                ops.normalize(feat.value.data, _norm_value(feat.norm), use_abs=False)
            return out
        pool = self.__dict__.setdefault("_bits_pool", {})

        def scratch(key, shape, dtype, dev):
            t = pool.get(key)
            if t is None or tuple(t.shape) != tuple(shape) or t.device != dev:
                t = pool[key] = torch.empty(shape, dtype=dtype, device=dev)
            return t
        prog = self._program(out.device, scratch, "hand")
        draws = [(f.value.data, bits) for kind, f, _, bits in prog if kind == _lib.MCC_OP_MUL_DRAW]
        if draws:                                   # the host generator goes to the device and comes back advanced (rng.py)
            ops.mcc_bernoulli_from_host([p for p, _ in draws], [b for _, b in draws], self.source.n, self.target.n)
        ops.prop_mcc_pipe([(kind, f.value.data, flag, bits) for kind, f, flag, bits in prog], s, out, self.source.n, self.target.n,
                          accumulate=accumulate)
        for f in self.pipeline:                     # a Weight with norm_frequency="time step": normalised behind the step's signal
            if getattr(f, "_norm_step", bool)():
                ops.normalize(f.value.data, _norm_value(f.norm), use_abs=False)

    def _host_update(self, kwargs, mask) -> None:
        host_path._update_mcc(self, float(self.dt), kwargs)

    def _host_normalize(self) -> None:
        for feat in self.pipeline:                    # topology.py:520-527: every feature that has a norm (a "time step" Weight: a no-op, topology_features.py:663-671)
            if feat.norm is not None and getattr(feat, "norm_frequency", "sample") == "sample":
                host_path._normalize_columns(feat.value.data, feat.norm, False)

    def _rule(self):
        from ..learning.MCC_learning import NoOp
        feat = self._learned()
        return NoOp() if feat is None else feat.learning_rule

    def _column_slice(self, source, target, lo, hi):
        from .topology_features import Weight
        feat = self._single_weight("column_shard")
        rule = feat.learning_rule
        from ..learning import MCC_learning
        rule_cls = type(rule) if type(rule) in (MCC_learning.PostPre, MCC_learning.MSTDP) else None
        lo_b, hi_b = (rule.min, rule.max) if rule_cls is not None else (-float("inf"), float("inf"))
        f2 = Weight(feat.name, feat.value.data[:, lo:hi].clone().cpu(), range=[lo_b, hi_b], norm=feat.norm,
                    nu=None if rule_cls is None else (float(rule.nu[0]), float(rule.nu[1])), learning_rule=rule_cls,
                    decay=0.0 if rule_cls is None or rule.decay == 1.0 else 1.0 - float(rule.decay))
        c2 = MulticompartmentConnection(source, target, device="cpu", pipeline=[f2], manual_update=self.manual_update)
        if rule_cls is not None:
            f2.learning_rule.reduction = rule.reduction
        return c2

    def _exact_learns(self) -> bool:
        from ..learning import MCC_learning
        rule = self._single_weight("exact_run").learning_rule
        if self.manual_update or isinstance(rule, MCC_learning.NoOp):
            return False
        if not isinstance(rule, MCC_learning.PostPre):
            raise NotImplementedError(f"exact_run: MCC rule {type(rule).__name__} (supported: PostPre)")
        if not (self.source.traces and self.target.traces):
            raise AssertionError("PostPre needs traces on both layers")
        return True

    def _weights(self):
        return self._weight(), "value"

    def _describe(self, d, B, dev, scratch):
        if not self._single():
            return self._describe_pipe(d, B, dev, scratch)
        feat = self.pipeline[0]
        if feat.value.device != dev:
            feat.to(dev)
        val = feat.value
        if (val.dtype != torch.float32 and val.dtype not in ops.HALF) or not val.is_contiguous() or \
                tuple(val.shape) != (self.source.n, self.target.n):
            raise NotImplementedError(f"bindsnet_amd: Weight.value must be a contiguous float32, float16 or bfloat16 [{self.source.n}, "
                                      f"{self.target.n}] tensor (got {val.dtype}, shape {tuple(val.shape)}, "
                                      f"contiguous={val.is_contiguous()})")
        _lib.raise_if(self._run_refusal(None, False))
        # (float16 / bfloat16: `w` points at 2-byte elements and the run takes the generic plan's *_h16 kernels, csrc/snn_half.hip)
        d.kind, d.w, d.w_dtype = self._kind, dptr(val.data), ops.HALF.get(val.dtype, _lib.W_F32)
        if feat.norm is not None:
            ws = scratch(f"norm_{d.src}_{d.dst}", (self.target.n,), torch.float32, dev)
            _fill_norm(d, feat.norm, 0, ws, self.target.n, dev)
            d.norm_step = self._NORM_STEP_FORM if feat._norm_step() else 0
        return [self._weights()] + self._activity_buffer(d, B, dev)

    def _describe_pipe(self, d, B, dev, scratch):
        """The feature program at the end of snn_conn_desc; d.w is the Weight the rule and the norm refer to (NULL without one)."""
        from .topology_features import Weight
        prog = self._program(dev, scratch, f"{d.src}_{d.dst}")
        feat = self._learned()
        d.kind, d.pipe_n = self._kind, len(prog)
        described = []
        for k, (kind, f, flag, bits) in enumerate(prog):
            d.pipe_kind[k], d.pipe_val[k], d.pipe_scalar[k], d.pipe_bits[k] = kind, f.value.data_ptr(), flag, 0 if bits is None else bits.data_ptr()
            described.append((f, "value"))
            if f is not feat and f.norm is not None:
                raise NotImplementedError("bindsnet_amd: in a feature pipeline only the Weight the rule refers to may have a norm on the device")
        if feat is not None:
            if tuple(feat.value.shape) != (self.source.n, self.target.n):
                raise NotImplementedError("bindsnet_amd: the Weight of a pipeline must be a [source.n, target.n] tensor")
            d.w = dptr(feat.value.data)
            if feat.norm is not None:
                ws = scratch(f"norm_{d.src}_{d.dst}", (self.target.n,), torch.float32, dev)
                _fill_norm(d, feat.norm, 0, ws, self.target.n, dev)
                d.norm_step = int(feat._norm_step())      # (snn_prop_mcc_pipe_f32, then the normalisation: the two-call form)
        return described + self._activity_buffer(d, B, dev)

    def update(self, **kwargs) -> None:
        """Reference: topology.py:509-518 (note the default learning=False)."""
        if kwargs.get("learning", False) and not self.manual_update:
            if self._on_host():                         # a connection on the host: plain PyTorch (network/host_path.py)
                return self._host_update(kwargs, None)
            for f in self.pipeline:
                f.update(**kwargs)

    def normalize(self) -> None:
        if self._on_host():
            return self._host_normalize()
        for f in self.pipeline:
            f.normalize()

    def reset_state_variables(self) -> None:
        for f in self.pipeline:
            f.reset_state_variables()
