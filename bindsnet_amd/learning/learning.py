"""Learning rules for dense `Connection`s: API mirror of bindsnet/learning/learning.py for `LearningRule`, `NoOp`,
`PostPre`, `WeightDependentPostPre`, `Hebbian`, `MSTDP`, `MSTDPET`, `Rmax`.  Updates run in snn_stdp_postpre /
snn_stdp_hebbian / snn_mstdp_step / snn_mstdpet_step / snn_rmax_step (on a Conv2dConnection: snn_conv2d_postpre / snn_conv2d_hebbian /
snn_conv2d_mstdp_step)."""
import warnings
from typing import Optional, Sequence, Union

import numpy as np
import torch

from ..network.nodes import _f

from .. import _lib
from . import _descriptor


class LearningRule(_descriptor.Rule):
    """Reference: learning.py:25-104.  Which rules a connection family takes is the family's `_rules` (network/topology.py)."""

    _rule_code = None                       # snn_conn_desc.rule (include/snnhip.h)

    def __init__(self, connection, nu: Optional[Union[float, Sequence[float], Sequence[torch.Tensor]]] = None,
                 reduction: Optional[callable] = None, weight_decay: float = 0.0, **kwargs) -> None:
        if getattr(connection, "_rules_only", None) and not _descriptor.accepts(connection, self):
            raise NotImplementedError(f"bindsnet_amd: {type(self).__name__} on {type(connection).__name__} is not supported "
                                      f"({connection._rules_only})")
        _lib.raise_if(connection._rule_refusal(self))   # a family's own reason against this rule (Conv2dConnection: wide inputs)
        self.connection = connection
        self.source, self.target = connection.source, connection.target
        self.wmin, self.wmax = connection.wmin, connection.wmax
        if nu is None:
            self.nu = torch.tensor([0.0, 0.0], dtype=torch.float)
        elif isinstance(nu, (float, int)):
            self.nu = torch.tensor([nu, nu], dtype=torch.float)
        elif all(isinstance(e, (float, int)) for e in nu):
            self.nu = torch.tensor(nu, dtype=torch.float)
        elif connection._kind != _lib.CONN_DENSE or self._rule_code in (None, _lib.RULE_RMAX):
            raise NotImplementedError("bindsnet_amd: per-synapse tensor learning rates are not supported")
        else:                                   # learning.py:67: a pair of tensors, each broadcast against the [source.n, target.n] weights
            self.nu = torch.stack(nu, dim=0).to(dtype=torch.float)
            if self.nu[0].numel() > 1:
                self.nu[0].expand(self.source.n, self.target.n)     # (what does not broadcast: torch's RuntimeError, as in the first update)
        if not self.nu.any() and not isinstance(self, NoOp):
            warnings.warn(f"nu is set to zeros for {type(self).__name__} learning rule. "
                          "It will disable the learning process.")
        if reduction is None:  # learning.py:76-82
            reduction = torch.squeeze if self.source.batch_size == 1 else torch.sum
        self.reduction = reduction
        self.weight_decay = 1.0 - weight_decay if weight_decay else 1.0

    @property
    def _takes_syn(self) -> bool:
        """Whether the rule's updates take per-synapse constants (the *_pv entry points): the dense family's rules but Rmax."""
        return self.connection._kind == _lib.CONN_DENSE and self._rule_code not in (None, _lib.RULE_NONE, _lib.RULE_RMAX)

    def _nu(self, i: int):
        """Learning rate i as the ops take it: a float, or the tensor of more than one element."""
        kept = self.__dict__.get("_nu_views")          # the SAME view objects from call to call: the device copy and `.any()` are
        if kept is None or kept[0] is not self.nu or kept[1][0]._base is not self.nu:    # remembered on them, keyed by the in-place version
            # they share with `nu` (a copy or an unpickled rule has tensors of its own, no longer views of its `nu`: made again)
            kept = (self.nu, (self.nu[0], self.nu[1]))
            self.__dict__["_nu_views"] = kept
        t = kept[1][i]
        return t if t.numel() > 1 else float(t)

    def _bounds(self, tensors: bool = False):
        """(lower, upper) clamp bound: None where there is none, a float, or -- `tensors`, for the callers that hand them on to the
        *_pv entry points -- a tensor of more than one element."""
        c = self.connection
        if c.wmin.numel() != 1 or c.wmax.numel() != 1:
            if not (tensors and self._takes_syn):
                raise NotImplementedError("bindsnet_amd: per-synapse wmin/wmax tensors are not supported")

            def one(t, inf):
                if t.numel() > 1:
                    return t
                v = _f(t)
                return None if v == inf else v
            return one(c.wmin, -np.inf), one(c.wmax, np.inf)
        lo, hi = _f(c.wmin), _f(c.wmax)      # (through _f: an in-place edit of the bounds invalidates the kept run descriptors)
        clamp = (lo != -np.inf or hi != np.inf) and not isinstance(self, NoOp)   # learning.py:97-104
        if not clamp:
            return None, None
        return (None if lo == -np.inf else lo), (None if hi == np.inf else hi)

    def _check_reduction(self):
        B = self.source.batch_size
        if self.reduction is torch.squeeze:
            if B != 1:
                raise RuntimeError("reduction=torch.squeeze with batch size > 1: pass reduction=torch.sum "
                                   "(the reference fails with a broadcast error here)")
        else:
            _descriptor.check_reduction(self)

    def _reduce(self) -> str:
        """The batch reduction as the ops take it ("sum", "mean", "amax", "amin")."""
        return _descriptor.reduce_of(self, self.source.batch_size)

    def _require_accepted(self) -> None:
        if not _descriptor.accepts(self.connection, self):
            raise NotImplementedError("This learning rule is not supported for this Connection type.")

    def _describe(self, d, conn, B, dev, keep, kwargs) -> None:
        """Write the rule's fields of the connection's snn_conn_desc `d` for a Network.run at batch size B: here what
        PostPre, Hebbian and WeightDependentPostPre need (use_dt stays 0), and what MSTDP starts with."""
        if self._rule_code is None:
            raise NotImplementedError(f"bindsnet_amd: rule {type(self).__name__} is not supported")
        self._check_reduction()
        _lib.raise_if(self._syn_refusal())
        _descriptor.fill_update(d, self, self.weight_decay, dev, keep)
        d.rule = self._rule_code
        # (anything but sum: the generic plan, the *_red entry points; a rule that reduces nothing keeps every plan)
        d.reduce = _lib.REDUCE["sum" if self._rule_code == _lib.RULE_NONE else _descriptor.reduce_of(self, B)]

    def update(self, **kwargs) -> None:
        raise NotImplementedError

    def reset_state_variables(self) -> None:
        pass


class NoOp(LearningRule):
    _rule_code, _learns = _lib.RULE_NONE, False

    def update(self, **kwargs) -> None:
        if self.weight_decay != 1.0:
            raise NotImplementedError("bindsnet_amd: weight_decay without a learning rule is not supported")


class PostPre(LearningRule):
    """Reference: learning.py:149-206, _connection_update :390-420 (the device op is the connection family's `_postpre`)."""

    _rule_code = _lib.RULE_POSTPRE

    def __init__(self, connection, nu=None, reduction=None, weight_decay: float = 0.0, **kwargs) -> None:
        super().__init__(connection=connection, nu=nu, reduction=reduction, weight_decay=weight_decay, **kwargs)
        assert self.source.traces and self.target.traces, "Both pre- and post-synaptic nodes must record spike traces."
        self._require_accepted()
        _lib.raise_if(self._syn_refusal())

    def _syn_refusal(self):
        """learning.py:401-402: `target_x * nu[0]` must stay [B, 1, N] for the bmm -- rates that vary along the source axis fail there."""
        for i in (0, 1):
            t = self.nu[i]
            if t.numel() > 1 and (t.dim() > 2 or (t.dim() == 2 and t.shape[0] != 1)):
                return RuntimeError(f"PostPre: nu[{i}] of shape {list(t.shape)} does not broadcast against the [batch, 1, {self.target.n}] "
                                    "target factor (batch2 of the bmm at learning.py:402 / :414 must stay a 3D tensor of that shape)")
        return None

    def update(self, **kwargs) -> None:
        self._check_reduction()
        _lib.raise_if(self._syn_refusal())
        self.connection._postpre(self, self.source.batch_size, *self._bounds(tensors=True))


class MSTDP(LearningRule):
    """Reward-modulated STDP (reference: learning.py:1441-1574).  The dense eligibility tensor of the
    reference is kept factored on the device (see snn_mstdp_step); `p_plus`, `p_minus` keep their
    reference meaning.

    On a Conv2dConnection (learning.py:1942-2015; snn_conv2d_mstdp_step) the rule is defined at batch size 1, like the
    reference's (its `eligibility.view(w.size())`, :2013, admits no other); `eligibility` is then the rule's dense
    [Cout, Cin, KH, KW] state, `p_minus` is [Cout, OH*OW] and `p_plus` is kept in INPUT space [Cin, H, W] -- the
    reference's attribute is its im2col (`bindsnet.utils.im2col_indices(rule.p_plus[None], ...)` gives that layout)."""

    _rule_code = _lib.RULE_MSTDP

    def __init__(self, connection, nu=None, reduction=None, weight_decay: float = 0.0, **kwargs) -> None:
        super().__init__(connection=connection, nu=nu, reduction=reduction, weight_decay=weight_decay, **kwargs)
        self._require_accepted()
        self._conv = connection._kind == _lib.CONN_CONV2D
        self.tc_plus = torch.tensor(kwargs.get("tc_plus", 20.0))
        self.tc_minus = torch.tensor(kwargs.get("tc_minus", 20.0))

    def _ensure_state(self):
        if self._conv:
            w = self.connection.w
            if not hasattr(self, "p_plus") or self.p_plus.device != w.device:
                self.p_plus = torch.zeros(*self.source.shape, device=w.device)
                self.p_minus = torch.zeros(w.shape[0], self.target.n // w.shape[0], device=w.device)
                self._elig = torch.zeros_like(w.data)
            return
        B, dev = self.source.batch_size, self.connection.w.device
        if not hasattr(self, "p_plus") or self.p_plus.shape[0] != B or self.p_plus.device != dev:
            self.p_plus = torch.zeros(B, self.source.n, device=dev)
            self.p_minus = torch.zeros(B, self.target.n, device=dev)
            self._s_src_prev = torch.zeros(B, self.source.n, dtype=torch.uint8, device=dev)
            self._s_tgt_prev = torch.zeros(B, self.target.n, dtype=torch.uint8, device=dev)

    def _decays(self):
        dt = torch.tensor(self.connection.dt)
        return float(torch.exp(-dt / self.tc_plus)), float(torch.exp(-dt / self.tc_minus))   # learning.py:1564,1566

    def _conv_reward(self, B, kwargs) -> float:
        if B != 1:
            raise NotImplementedError("MSTDP on a Conv2dConnection is defined for batch size 1 (learning.py:2013)")
        reward = _descriptor.reward(kwargs)
        if isinstance(reward, torch.Tensor):
            if reward.numel() != 1:
                raise NotImplementedError("bindsnet_amd: MSTDP on a Conv2dConnection takes a scalar reward")
            reward = reward.item()
        return float(reward)

    def _describe(self, d, conn, B, dev, keep, kwargs) -> None:
        super()._describe(d, conn, B, dev, keep, kwargs)
        if not self._conv:
            return _descriptor.fill_mstdp(d, self, kwargs, dev, keep)
        d.reward = self._conv_reward(B, kwargs)                                    # learning.py:1942-2015, batch 1
        d.reduce = _lib.REDUCE["sum"]                                              # (:2013 hard-codes torch.sum: `reduction` is ignored)
        d.a_plus, d.a_minus = _descriptor.a_plus_minus(kwargs)
        self._ensure_state()
        d.decay_plus, d.decay_minus = self._decays()
        d.p_plus, d.p_minus, d.e_trace = _lib.dptr(self.p_plus), _lib.dptr(self.p_minus), _lib.dptr(self._elig)

    def _conv_update(self, **kwargs) -> None:
        from .. import ops
        reward = self._conv_reward(self.source.batch_size, kwargs)
        self._ensure_state()
        dp, dm = self._decays()
        lo, hi = self._bounds()
        c = self.connection
        ops.conv2d_mstdp_step(c.w.data, self._elig, self.p_plus, self.p_minus, self.source.s.contiguous(), self.target.s.contiguous(),
                              reward, float(self.nu[0]), float(kwargs.get("a_plus", 1.0)), float(kwargs.get("a_minus", -1.0)),
                              dp, dm, stride=c.stride[0], pad=c.padding[0], wdecay=float(self.weight_decay), wmin=lo, wmax=hi)

    def update(self, **kwargs) -> None:
        from .. import ops
        if self._conv:
            return self._conv_update(**kwargs)
        self._check_reduction()
        self._ensure_state()
        B = self.source.batch_size
        reward, rvec = _descriptor.split_reward(kwargs["reward"], self.connection.w.device)
        dp, dm = self._decays()
        lo, hi = self._bounds(tensors=True)
        ops.mstdp_step(self.connection.w.data, self.p_plus, self.p_minus, self._s_src_prev, self._s_tgt_prev,
                       self.source.s.reshape(B, -1).contiguous(), self.target.s.reshape(B, -1), reward,
                       self._nu(0), float(kwargs.get("a_plus", 1.0)), float(kwargs.get("a_minus", -1.0)), dp, dm,
                       wdecay=float(self.weight_decay), wmin=lo, wmax=hi, reward_vec=rvec, reduce=self._reduce())

    @property
    def eligibility(self) -> torch.Tensor:
        """Dense view of the factored eligibility (for inspection only); the rule's own state on a Conv2dConnection."""
        self._ensure_state()
        if self._conv:
            return self._elig
        return (self.p_plus.unsqueeze(2) * self._s_tgt_prev.float().unsqueeze(1)
                + self._s_src_prev.float().unsqueeze(2) * self.p_minus.unsqueeze(1))


class _OuterProductRule(LearningRule):
    """Shared part of Hebbian / WeightDependentPostPre: raw outer products reduced over the batch, then scaled."""
    _weight_dependent = False

    def __init__(self, connection, nu=None, reduction=None, weight_decay: float = 0.0, **kwargs) -> None:
        super().__init__(connection=connection, nu=nu, reduction=reduction, weight_decay=weight_decay, **kwargs)
        self._require_accepted()

    def update(self, **kwargs) -> None:
        from .. import ops
        self._check_reduction()
        B = self.source.batch_size
        if self.connection._kind == _lib.CONN_CONV2D:
            return self.connection._outer_product(self, B, *self._bounds())
        _lib.raise_if(self._syn_refusal())
        lo, hi = self._bounds(tensors=True)
        ops.stdp_hebbian(self.connection.w.data, self.source.s.reshape(B, -1).contiguous(), self.source.x.reshape(B, -1),
                         self.target.s.reshape(B, -1), self.target.x.reshape(B, -1), self._nu(0), self._nu(1),
                         weight_dependent=self._weight_dependent, decay=float(self.weight_decay), wmin=lo, wmax=hi, reduce=self._reduce())


class Hebbian(_OuterProductRule):
    """Both the pre- and the post-synaptic term potentiate (reference: learning.py:1052-1135; on a Conv2dConnection :1348-1380)."""
    _rule_code = _lib.RULE_HEBBIAN

    def __init__(self, connection, nu=None, reduction=None, weight_decay: float = 0.0, **kwargs) -> None:
        super().__init__(connection=connection, nu=nu, reduction=reduction, weight_decay=weight_decay, **kwargs)
        assert self.source.traces and self.target.traces, "Both pre- and post-synaptic nodes must record spike traces."


class WeightDependentPostPre(_OuterProductRule):
    """PostPre whose depression scales with (w - wmin) and potentiation with (wmax - w) (reference: learning.py:562-653; on a Conv2dConnection
    :920-976)."""
    _rule_code, _weight_dependent = _lib.RULE_WDPOSTPRE, True

    def __init__(self, connection, nu=None, reduction=None, weight_decay: float = 0.0, **kwargs) -> None:
        super().__init__(connection=connection, nu=nu, reduction=reduction, weight_decay=weight_decay, **kwargs)
        assert self.source.traces, "Pre-synaptic nodes must record spike traces."
        assert (connection.wmin != -np.inf).any() and (connection.wmax != np.inf).any(), \
            "Connection must define finite wmin and wmax."
        if not self.target.traces:
            raise NotImplementedError("bindsnet_amd: WeightDependentPostPre needs spike traces on the target layer too "
                                      "(the update reads target.x)")
        _lib.raise_if(self._syn_refusal())

    def _syn_refusal(self):
        """A bound tensor with a non-finite entry passes the reference's `.any()` assertion and turns the weights into NaN."""
        c = self.connection
        for t in (c.wmin, c.wmax):
            if t.numel() > 1 and not _descriptor.all_finite(t):
                return NotImplementedError("bindsnet_amd: WeightDependentPostPre needs finite wmin and wmax for every synapse "
                                           "(a bound tensor has a non-finite entry)")
        return None


class MSTDPET(LearningRule):
    """Reward-modulated STDP with an eligibility trace (reference: learning.py:2124-2248); like the reference's dense
    form it is defined for batch size 1.  `eligibility_trace` is the rule's dense [Nin, N] state on the device."""

    _rule_code = _lib.RULE_MSTDPET

    def __init__(self, connection, nu=None, reduction=None, weight_decay: float = 0.0, **kwargs) -> None:
        super().__init__(connection=connection, nu=nu, reduction=reduction, weight_decay=weight_decay, **kwargs)
        self._require_accepted()
        self.tc_plus = torch.tensor(kwargs.get("tc_plus", 20.0))
        self.tc_minus = torch.tensor(kwargs.get("tc_minus", 20.0))
        self.tc_e_trace = torch.tensor(kwargs.get("tc_e_trace", 25.0))

    def _ensure_state(self):
        dev = self.connection.w.device
        if not hasattr(self, "p_plus") or self.p_plus.device != dev:
            self.p_plus = torch.zeros(self.source.n, device=dev)
            self.p_minus = torch.zeros(self.target.n, device=dev)
            self.eligibility_trace = torch.zeros(*self.connection.w.shape, device=dev)
            self._s_src_prev = torch.zeros(self.source.n, dtype=torch.uint8, device=dev)
            self._s_tgt_prev = torch.zeros(self.target.n, dtype=torch.uint8, device=dev)

    def _decays(self):
        dt = torch.tensor(self.connection.dt)
        return (float(torch.exp(-dt / self.tc_plus)), float(torch.exp(-dt / self.tc_minus)),
                float(torch.exp(-dt / self.tc_e_trace)))

    @property
    def eligibility(self) -> torch.Tensor:
        self._ensure_state()
        return torch.outer(self.p_plus, self._s_tgt_prev.float()) + torch.outer(self._s_src_prev.float(), self.p_minus)

    def _describe(self, d, conn, B, dev, keep, kwargs) -> None:
        if B != 1:
            raise NotImplementedError("MSTDPET on a dense Connection is defined for batch size 1 (learning.py:2211-2212)")
        _descriptor.fill_mstdpet(d, self, self.weight_decay, kwargs, dev, keep)

    def update(self, **kwargs) -> None:
        from .. import ops
        if self.source.batch_size != 1:
            raise NotImplementedError("MSTDPET on a dense Connection is defined for batch size 1 (learning.py:2211-2212)")
        self._ensure_state()
        dp, dm, de = self._decays()
        lo, hi = self._bounds(tensors=True)
        ops.mstdpet_step(self.connection.w.data, self.eligibility_trace, self.p_plus, self.p_minus, self._s_src_prev,
                         self._s_tgt_prev, self.source.s.reshape(-1).contiguous(), self.target.s.reshape(-1), float(kwargs["reward"]),
                         self._nu(0), float(self.connection.dt), float(kwargs.get("a_plus", 1.0)),
                         float(kwargs.get("a_minus", -1.0)), dp, dm, de, float(self.tc_e_trace),
                         wdecay=float(self.weight_decay), wmin=lo, wmax=hi)


class Rmax(LearningRule):
    """Reward-modulated rule derived from reward maximisation for stochastically firing neurons (reference: learning.py:2858-2960).
    Defined for `Connection` and `LocalConnection` into an `SRM0Nodes` layer, from a source with additive traces, at batch size
    1 (the reference flattens the target's state with `view(-1)`).  `eligibility_trace` is the rule's dense [source.n, target.n]
    state, created on first use."""

    _rule_code = _lib.RULE_RMAX
    _B1 = ("Rmax is defined for batch size 1 (learning.py:2940-2942: `target_s = self.target.s.view(-1).float()`, "
           "`target_s_prob = self.target.s_prob.view(-1)`, `source_x = self.source.x.view(-1)`)")

    def __init__(self, connection, nu=None, reduction=None, weight_decay: float = 0.0, **kwargs) -> None:
        if not _descriptor.accepts(connection, self) and not getattr(connection, "_rules_only", None):
            # (a family without the dense connections' attributes -- MulticompartmentConnection -- cannot reach the base constructor)
            raise NotImplementedError("This learning rule is not supported for this Connection type.")
        super().__init__(connection=connection, nu=nu, reduction=reduction, weight_decay=weight_decay, **kwargs)
        from ..network.nodes import SRM0Nodes
        assert self.source.traces and self.source.traces_additive, "Pre-synaptic nodes must use additive spike traces."
        assert isinstance(self.target, SRM0Nodes), "R-max needs stochastically firing neurons, use SRM0Nodes."
        self._require_accepted()
        self.tc_c = torch.tensor(kwargs.get("tc_c", 5.0))
        self.tc_e_trace = torch.tensor(kwargs.get("tc_e_trace", 25.0))

    def _batch_refusal(self, B: int):
        return NotImplementedError(self._B1) if B != 1 else None

    def _multi_device_refusal(self, mode, key):
        return NotImplementedError(f"{mode}: Rmax on connection {key} is not supported by the multi-device modes (the rule is defined for "
                                   "batch size 1 and reads a layer that draws from the host generator); run the network on one device")

    def _ensure_state(self) -> None:
        w = self.connection.w
        t = self.__dict__.get("eligibility_trace")
        if t is None:
            self.eligibility_trace = torch.zeros(*w.shape, device=w.device)
        elif t.device != w.device:
            self.eligibility_trace = t.to(w.device)

    @staticmethod
    def _reward(kwargs) -> float:
        r = _descriptor.reward(kwargs)
        if isinstance(r, torch.Tensor):
            if r.numel() != 1:
                raise NotImplementedError("bindsnet_amd: Rmax takes a scalar reward (the rule is defined for batch size 1)")
            return float(r.reshape(()).item())
        if not isinstance(r, (int, float)):
            raise NotImplementedError(f"bindsnet_amd: Rmax takes a scalar reward, got {type(r).__name__}")
        return float(r)

    def _describe(self, d, conn, B, dev, keep, kwargs) -> None:
        if B != 1:
            raise NotImplementedError(self._B1)
        reward = self._reward(kwargs)
        self._ensure_state()
        _descriptor.fill_update(d, self, self.weight_decay)
        d.rule, d.reward = self._rule_code, reward
        d.tc_e, d.rmax_tc_c = float(self.tc_e_trace), float(self.tc_c)
        d.e_trace = _lib.dptr(self.eligibility_trace)

    def update(self, **kwargs) -> None:
        from .. import ops
        if self.source.batch_size != 1:
            raise NotImplementedError(self._B1)
        reward = self._reward(kwargs)
        self._ensure_state()
        lo, hi = self._bounds()
        c = self.connection
        ops.rmax_step(c.w.data.view(self.source.n, self.target.n), self.eligibility_trace, self.target.s.reshape(-1).contiguous(),
                      self.target.s_prob.reshape(-1), self.source.x.reshape(-1), reward, float(self.nu[0]), float(c.dt),
                      float(self.tc_c), float(self.tc_e_trace), wdecay=float(self.weight_decay), wmin=lo, wmax=hi)
