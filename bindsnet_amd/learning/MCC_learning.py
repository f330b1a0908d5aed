"""Learning rules for MulticompartmentConnection features: API mirror of
bindsnet/learning/MCC_learning.py for `MCC_LearningRule`, `NoOp`, `PostPre`, `MSTDP`, `MSTDPET`.
The updates themselves are snn_stdp_postpre (use_dt = 1; snn_stdp_postpre_h16 on a float16 / bfloat16 Weight) / snn_mstdp_step /
snn_mstdpet_step; with average_update > 0 their ring forms snn_postpre_avg_step / snn_mstdp_avg_step / snn_mstdpet_avg_step
(include/snnhip.h f14)."""
import warnings
from typing import Optional, Sequence, Union

import torch

from .. import _lib
from . import _descriptor


class MCC_LearningRule(_descriptor.Rule):
    """Reference: MCC_learning.py:16-118 (nu parsing, reduction default, decay, clamp range)."""

    _rule_code = None                  # snn_conn_desc.rule (include/snnhip.h)

    def __init__(self, connection, feature_value, range: Optional[Union[list, tuple]] = None,
                 nu: Optional[Union[float, Sequence[float]]] = None, reduction: Optional[callable] = None,
                 decay: float = 0.0, enforce_polarity: bool = False, **kwargs) -> None:
        self.connection = connection
        self.source, self.target = connection.source, connection.target
        self.feature_value = feature_value
        self.enforce_polarity = enforce_polarity
        if enforce_polarity:
            raise NotImplementedError("bindsnet_amd: enforce_polarity is outside the accelerated path")
        self.min, self.max = range
        if nu is None:
            nu = [0.2, 0.1]
        elif isinstance(nu, (float, int)):
            nu = [nu, nu]
        self.nu = torch.zeros(2, dtype=torch.float)
        self.nu[0], self.nu[1] = nu[0], nu[1]
        if (self.nu == torch.zeros(2)).all() and not isinstance(self, NoOp):
            warnings.warn(f"nu is set to [0., 0.] for {type(self).__name__} learning rule. "
                          "It will disable the learning process.")
        # MCC_learning.py:75-81: batch reduction defaults to sum unless the source already has batch 1
        if reduction is None:
            reduction = torch.squeeze if self.source.batch_size == 1 else torch.sum
        self.reduction = reduction
        self.decay = 1.0 - decay if decay else 1.0

    # ---- average_update / continues_update (MCC_learning.py:182-183, :211-222, :457-466, :641-649) ----------------------------
    _RINGS = ()                        # (ring attribute, index attribute, index of the learning rate its term runs on) per ring

    def _init_average(self, kwargs) -> None:
        """The reference's keyword arguments, rings and indices under its attribute names.  The rings are float32 zeros beside the
        weights and are never cleared by the rule (reset_state_variables leaves them alone, :304, :550, :735-738).  What the
        device path does not run is refused here, before anything exists."""
        K = kwargs.get("average_update", 0)
        if isinstance(K, bool) or not isinstance(K, int):
            raise TypeError(f"bindsnet_amd: average_update must be an int (got {K!r})")
        if K < 0:
            raise NotImplementedError(f"bindsnet_amd: average_update={K} is negative: it is the number of updates to average over "
                                      "(0: no averaging)")
        if K > _lib.AVG_MAX_TERMS:
            raise NotImplementedError(f"bindsnet_amd: average_update={K} is above the {_lib.AVG_MAX_TERMS} terms the ordered accumulator "
                                      "of the ring's mean takes (SNN_AVG_MAX_TERMS)")
        if K > 0:
            dtype = getattr(self.feature_value, "dtype", torch.float32)
            if dtype in (torch.float16, torch.bfloat16):
                raise NotImplementedError(f"bindsnet_amd: average_update on a {dtype} Weight is not supported: the ring and its mean "
                                          "are float32 and the reference's roundings of a half-precision ring are not restated")
            if _descriptor.is_vec(self.min) or _descriptor.is_vec(self.max):
                raise NotImplementedError("bindsnet_amd: average_update with tensor (per-synapse) clamp ranges is not supported: the "
                                          "averaged entry points take scalar bounds")
        self.average_update, self.continues_update = K, kwargs.get("continues_update", False)
        if K > 0:
            for ring, index, _ in self._RINGS:
                setattr(self, ring, torch.zeros(K, *self.feature_value.shape, device=self.feature_value.device))
                setattr(self, index, 0)

    def _move_rings(self, device) -> None:
        """The rings follow the Weight's value (AbstractFeature.to)."""
        if getattr(self, "average_update", 0):
            for ring, _, _ in self._RINGS:
                if getattr(self, ring).device != torch.device(device):
                    setattr(self, ring, getattr(self, ring).to(device))

    def _avg_indices(self):
        """The ring indices at the start of the next step, one per ring."""
        return [int(getattr(self, index)) for _, index, _ in self._RINGS]

    def _avg_advance(self, steps: int = 1) -> None:
        """`steps` learning steps have run: every ring has moved on, but a PostPre term whose rate is 0 never runs (:233, :267)."""
        for _, index, rate in self._RINGS:
            if rate is None or float(self.nu[rate]) != 0.0:
                setattr(self, index, (int(getattr(self, index)) + steps) % self.average_update)

    def _describe_average(self, d, dev, keep, squeeze: bool) -> None:
        """The averaging fields of snn_conn_desc; the start indices are per-call values, bound by Network.run (_bind_call)."""
        if not getattr(self, "average_update", 0):
            return
        if _descriptor.is_vec(self.min) or _descriptor.is_vec(self.max):
            raise NotImplementedError("bindsnet_amd: average_update with tensor (per-synapse) clamp ranges is not supported: the "
                                      "averaged entry points take scalar bounds")
        self._move_rings(dev)
        rings = [getattr(self, ring) for ring, _, _ in self._RINGS]
        d.avg_k, d.avg_continuous, d.avg_squeeze = self.average_update, int(bool(self.continues_update)), int(squeeze)
        d.avg_ring0 = _lib.dptr(rings[0])
        d.avg_ring1 = _lib.dptr(rings[1]) if len(rings) > 1 else None
        keep.extend(rings)

    def _float32_only(self) -> None:
        """The reward-modulated rules keep float32 state beside the weights: a float16 / bfloat16 Weight is refused by name."""
        dtype = getattr(self.feature_value, "dtype", torch.float32)
        if dtype in (torch.float16, torch.bfloat16):
            raise NotImplementedError(f"bindsnet_amd: MCC {type(self).__name__} on a {dtype} Weight is not supported "
                                      "(NoOp and PostPre are)")

    @property
    def _takes_syn(self) -> bool:
        """Whether the rule's updates take per-synapse clamp ranges (the *_pv entry points): a float32 Weight."""
        return getattr(self.feature_value, "dtype", torch.float32) == torch.float32

    def _nu(self, i: int) -> float:
        return float(self.nu[i])           # (MCC_learning.py:64-66 keeps a 2-vector: tensor rates fail in the constructor)

    def _bounds(self, tensors: bool = False):
        """(lower, upper) clamp bound: None, a float or -- `tensors`, for the callers that hand them on to the *_pv entry points
        -- a tensor of more than one element (range=[tensor, tensor], MCC_learning.py:52, :110)."""
        def one(v):
            if v is None:
                return None
            if isinstance(v, torch.Tensor):
                if v.numel() != 1:
                    if tensors and self._takes_syn:
                        return v
                    raise NotImplementedError("bindsnet_amd: per-synapse clamp ranges are not supported")
                v = v.item()
            v = float(v)
            return None if v in (float("inf"), float("-inf")) else v
        return one(self.min), one(self.max)

    def _describe(self, d, conn, B, dev, keep, kwargs) -> None:
        """Write the rule's fields of the connection's snn_conn_desc `d` for a Network.run at batch size B.  A rule that
        does not say how is refused, and so is every rule but NoOp on a manual_update connection."""
        raise NotImplementedError(f"bindsnet_amd: MCC rule {type(self).__name__} is not supported")

    def _describe_batched(self, d, conn, B, dev=None, keep=None) -> None:
        """What PostPre and MSTDP share: the refusals, then bounds, decay and learning rates."""
        if conn.manual_update:
            MCC_LearningRule._describe(self, d, conn, B, None, None, None)
        if self.reduction is torch.squeeze and B != 1:
            raise RuntimeError("reduction=torch.squeeze requires batch size 1")
        _descriptor.fill_update(d, self, self.decay, dev, keep)
        d.reduce = _lib.REDUCE[_descriptor.reduce_of(self, B)]       # (checked here too: `reduction` may have been assigned since the constructor)

    def update(self, **kwargs) -> None:
        raise NotImplementedError

    def reset_state_variables(self) -> None:
        pass


class NoOp(MCC_LearningRule):
    _rule_code, _learns = _lib.RULE_NONE, False

    def __init__(self, **args) -> None:
        pass

    def update(self, **kwargs) -> None:
        pass

    def reset_state_variables(self) -> None:
        pass


class PostPre(MCC_LearningRule):
    """STDP with pre- (depressing) and post-synaptic (potentiating) terms.
    Reference: MCC_learning.py:149-305."""

    def __init__(self, connection, feature_value, range=None, nu=None, reduction=None, decay: float = 0.0,
                 enforce_polarity: bool = False, **kwargs) -> None:
        super().__init__(connection=connection, feature_value=feature_value,
                         range=[-1, +1] if range is None else range, nu=nu, reduction=reduction, decay=decay,
                         enforce_polarity=enforce_polarity, **kwargs)
        assert self.source.traces and self.target.traces, (
            "Both pre- and post-synaptic nodes must record spike traces "
            "(use traces='True' on source/target layers)")
        from ..network.topology import MulticompartmentConnection
        if not isinstance(connection, MulticompartmentConnection):
            raise NotImplementedError("This learning rule is not supported for this Connection type.")
        _descriptor.check_reduction(self)
        self._init_average(kwargs)

    _RINGS = (("average_buffer_pre", "average_buffer_index_pre", 0), ("average_buffer_post", "average_buffer_index_post", 1))

    def _describe(self, d, conn, B, dev, keep, kwargs) -> None:
        self._describe_batched(d, conn, B, dev, keep)
        d.rule, d.use_dt = _lib.RULE_POSTPRE, 1
        self._describe_average(d, dev, keep, self.reduction is torch.squeeze)

    def update(self, **kwargs) -> None:
        """One step of MCC_learning.py:224-302 through the C ABI (used when a connection is
        updated by hand; Network.run drives the same kernel from C++)."""
        from .. import ops
        B = self.source.batch_size
        if self.reduction is torch.squeeze and B != 1:
            raise RuntimeError("reduction=torch.squeeze requires batch size 1 (as in the reference)")
        if self.average_update:                 # the ring form (snn_postpre_avg_step): scalar bounds
            lo, hi = self._bounds()
            self._move_rings(self.feature_value.device)
            i_pre, i_post = self._avg_indices()
            ops.postpre_avg_step(self.feature_value.data, self.source.s.reshape(B, -1).contiguous(), self.source.x.reshape(B, -1),
                                 self.target.s.reshape(B, -1), self.target.x.reshape(B, -1), float(self.nu[0]), float(self.nu[1]),
                                 float(self.connection.dt), self.average_buffer_pre, self.average_buffer_post, i_pre, i_post,
                                 bool(self.continues_update), squeeze=self.reduction is torch.squeeze, decay=float(self.decay),
                                 wmin=lo, wmax=hi, reduce=_descriptor.reduce_of(self, B))
            self._avg_advance()
            return
        lo, hi = self._bounds(tensors=True)
        ops.stdp_postpre(self.feature_value.data, self.source.s.reshape(B, -1).contiguous(),
                         self.source.x.reshape(B, -1), self.target.s.reshape(B, -1), self.target.x.reshape(B, -1),
                         float(self.nu[0]), float(self.nu[1]), use_dt=True, dt=float(self.connection.dt),
                         decay=float(self.decay), wmin=lo, wmax=hi, reduce=_descriptor.reduce_of(self, B))


class MSTDP(MCC_LearningRule):
    """Reward-modulated STDP on a MulticompartmentConnection's Weight (reference: MCC_learning.py:392-551).  Same
    arithmetic as the dense rule (learning.py:1504-1574); the dense eligibility tensor of the reference is kept factored
    on the device (snn_mstdp_step), `p_plus` / `p_minus` keep their reference meaning."""

    def __init__(self, connection, feature_value, range=None, nu=None, reduction=None, decay: float = 0.0,
                 enforce_polarity: bool = False, **kwargs) -> None:
        super().__init__(connection=connection, feature_value=feature_value,
                         range=[-1, +1] if range is None else range, nu=nu, reduction=reduction, decay=decay,
                         enforce_polarity=enforce_polarity, **kwargs)
        from ..network.topology import MulticompartmentConnection
        if not isinstance(connection, MulticompartmentConnection):
            raise NotImplementedError("This learning rule is not supported for this Connection type.")
        self._float32_only()
        _descriptor.check_reduction(self)
        self.tc_plus = torch.tensor(kwargs.get("tc_plus", 20.0))
        self.tc_minus = torch.tensor(kwargs.get("tc_minus", 20.0))
        self._init_average(kwargs)

    _RINGS = (("average_buffer", "average_buffer_index", None),)

    def _ensure_state(self):
        B, dev = self.source.batch_size, self.feature_value.device
        if not hasattr(self, "p_plus") or self.p_plus.shape[0] != B or self.p_plus.device != dev:
            self.p_plus = torch.zeros(B, self.source.n, device=dev)
            self.p_minus = torch.zeros(B, self.target.n, device=dev)
            self._s_src_prev = torch.zeros(B, self.source.n, dtype=torch.uint8, device=dev)
            self._s_tgt_prev = torch.zeros(B, self.target.n, dtype=torch.uint8, device=dev)

    def _decays(self):
        dt = self.connection.dt
        return float(torch.exp(-dt / self.tc_plus)), float(torch.exp(-dt / self.tc_minus))   # MCC_learning.py:538,540

    def _describe(self, d, conn, B, dev, keep, kwargs) -> None:
        self._describe_batched(d, conn, B, dev, keep)
        _descriptor.fill_mstdp(d, self, kwargs, dev, keep)
        self._describe_average(d, dev, keep, self.reduction is torch.squeeze)

    def update(self, **kwargs) -> None:
        from .. import ops
        B = self.source.batch_size
        if self.reduction is torch.squeeze and B != 1:
            raise RuntimeError("reduction=torch.squeeze requires batch size 1 (as in the reference)")
        self._ensure_state()
        reward, rvec = _descriptor.split_reward(kwargs["reward"], self.feature_value.device)
        dp, dm = self._decays()
        if self.average_update:                 # the ring form (snn_mstdp_avg_step): scalar bounds
            lo, hi = self._bounds()
            self._move_rings(self.feature_value.device)
            ops.mstdp_avg_step(self.feature_value.data, self.p_plus, self.p_minus, self._s_src_prev, self._s_tgt_prev,
                               self.source.s.reshape(B, -1).contiguous(), self.target.s.reshape(B, -1), reward, float(self.nu[0]),
                               float(kwargs.get("a_plus", 1.0)), float(kwargs.get("a_minus", -1.0)), dp, dm, self.average_buffer,
                               self._avg_indices()[0], bool(self.continues_update), squeeze=self.reduction is torch.squeeze,
                               wdecay=float(self.decay), wmin=lo, wmax=hi, reward_vec=rvec, reduce=_descriptor.reduce_of(self, B))
            self._avg_advance()
            return
        lo, hi = self._bounds(tensors=True)
        ops.mstdp_step(self.feature_value.data, self.p_plus, self.p_minus, self._s_src_prev, self._s_tgt_prev,
                       self.source.s.reshape(B, -1).contiguous(), self.target.s.reshape(B, -1), reward,
                       float(self.nu[0]), float(kwargs.get("a_plus", 1.0)), float(kwargs.get("a_minus", -1.0)), dp, dm,
                       wdecay=float(self.decay), wmin=lo, wmax=hi, reward_vec=rvec, reduce=_descriptor.reduce_of(self, B))

    @property
    def eligibility(self) -> torch.Tensor:
        """Dense view of the factored eligibility (for inspection only)."""
        self._ensure_state()
        return (self.p_plus.unsqueeze(2) * self._s_tgt_prev.float().unsqueeze(1)
                + self._s_src_prev.float().unsqueeze(2) * self.p_minus.unsqueeze(1))


class MSTDPET(MCC_LearningRule):
    """Reward-modulated STDP with an eligibility trace on a MulticompartmentConnection's Weight (reference:
    MCC_learning.py:554-733).  Same arithmetic as the dense rule (learning.py:2187-2248, snn_mstdpet_step) and, like it,
    defined for batch size 1 (the spikes are flattened, :665-666).  `eligibility_trace` is the rule's dense [Nin, N]
    state on the device; the point eligibility is kept as its two factors."""

    def __init__(self, connection, feature_value, range=None, nu=None, reduction=None, decay: float = 0.0,
                 enforce_polarity: bool = False, **kwargs) -> None:
        super().__init__(connection=connection, feature_value=feature_value,
                         range=[-1, +1] if range is None else range, nu=nu, reduction=reduction, decay=decay,
                         enforce_polarity=enforce_polarity, **kwargs)
        from ..network.topology import MulticompartmentConnection
        if not isinstance(connection, MulticompartmentConnection):
            raise NotImplementedError("This learning rule is not supported for this Connection type.")
        self._float32_only()
        self.tc_plus = torch.tensor(kwargs.get("tc_plus", 20.0))
        self.tc_minus = torch.tensor(kwargs.get("tc_minus", 20.0))
        self.tc_e_trace = torch.tensor(kwargs.get("tc_e_trace", 25.0))
        self._init_average(kwargs)

    _RINGS = (("average_buffer", "average_buffer_index", None),)

    def _ensure_state(self):
        dev = self.feature_value.device
        if not hasattr(self, "p_plus") or self.p_plus.device != dev:
            self.p_plus = torch.zeros(self.source.n, device=dev)
            self.p_minus = torch.zeros(self.target.n, device=dev)
            self.eligibility_trace = torch.zeros(*self.feature_value.shape, device=dev)
            self._s_src_prev = torch.zeros(self.source.n, dtype=torch.uint8, device=dev)
            self._s_tgt_prev = torch.zeros(self.target.n, dtype=torch.uint8, device=dev)

    def _decays(self):
        dt = torch.as_tensor(self.connection.dt, dtype=torch.float32)
        return (float(torch.exp(-dt / self.tc_plus)), float(torch.exp(-dt / self.tc_minus)),       # MCC_learning.py:711,713
                float(torch.exp(-dt / self.tc_e_trace)))                                           # :684-686

    @property
    def eligibility(self) -> torch.Tensor:
        """Dense view of the point eligibility (MCC_learning.py:724-726), for inspection only."""
        self._ensure_state()
        return torch.outer(self.p_plus, self._s_tgt_prev.float()) + torch.outer(self._s_src_prev.float(), self.p_minus)

    def _describe(self, d, conn, B, dev, keep, kwargs) -> None:
        if conn.manual_update:
            super()._describe(d, conn, B, dev, keep, kwargs)
        if B != 1:
            raise NotImplementedError("MCC MSTDPET is defined for batch size 1 (MCC_learning.py:665-666)")
        _descriptor.fill_mstdpet(d, self, self.decay, kwargs, dev, keep)
        self._describe_average(d, dev, keep, False)

    def update(self, **kwargs) -> None:
        from .. import ops
        if self.source.batch_size != 1:
            raise NotImplementedError("MCC MSTDPET is defined for batch size 1 (MCC_learning.py:665-666)")
        self._ensure_state()
        dp, dm, de = self._decays()
        if self.average_update:                 # the ring form (snn_mstdpet_avg_step): scalar bounds
            lo, hi = self._bounds()
            self._move_rings(self.feature_value.device)
            ops.mstdpet_avg_step(self.feature_value.data, self.eligibility_trace, self.p_plus, self.p_minus, self._s_src_prev,
                                 self._s_tgt_prev, self.source.s.reshape(-1).contiguous(), self.target.s.reshape(-1),
                                 float(kwargs["reward"]), float(self.nu[0]), float(self.connection.dt), float(kwargs.get("a_plus", 1.0)),
                                 float(kwargs.get("a_minus", -1.0)), dp, dm, de, float(self.tc_e_trace), self.average_buffer,
                                 self._avg_indices()[0], bool(self.continues_update), wdecay=float(self.decay), wmin=lo, wmax=hi)
            self._avg_advance()
            return
        lo, hi = self._bounds(tensors=True)
        ops.mstdpet_step(self.feature_value.data, self.eligibility_trace, self.p_plus, self.p_minus, self._s_src_prev,
                         self._s_tgt_prev, self.source.s.reshape(-1).contiguous(), self.target.s.reshape(-1), float(kwargs["reward"]),
                         float(self.nu[0]), float(self.connection.dt), float(kwargs.get("a_plus", 1.0)),
                         float(kwargs.get("a_minus", -1.0)), dp, dm, de, float(self.tc_e_trace),
                         wdecay=float(self.decay), wmin=lo, wmax=hi)

    def reset_state_variables(self) -> None:
        """MCC_learning.py:731-734: the point eligibility and its trace are cleared, P+ / P- are kept."""
        if hasattr(self, "p_plus"):
            self.eligibility_trace.zero_()
            self._s_src_prev.zero_()
            self._s_tgt_prev.zero_()
