"""Connection features: API mirror of bindsnet/network/topology_features.py for the features on
the hot path (`AbstractFeature`, `Weight`, `Probability`, `Mask`, `Bias`, `Intensity`).  A feature only holds its
[Nin, N] tensor (and, a `Weight`, its learning rule); what a pipeline of them computes runs in snn_prop_cascade_f32
(one `Weight`) or in snn_mcc_bernoulli + snn_prop_mcc_pipe_f32 (every other pipeline; csrc/snn_mccpipe.hip), and on the
host in network/host_path.py."""
import warnings
from typing import Optional, Sequence, Union

import torch
from torch.nn import Parameter

from .. import _lib


class AbstractFeature(_lib.Touching):
    """Reference: topology_features.py:15-362 (constructor contract, priming, normalisation)."""

    def __init__(self, name: str, value=None, value_dtype: torch.dtype = torch.float32, range=None,
                 clamp_frequency: Optional[int] = 1, norm=None, learning_rule=None, nu=None, reduction=None,
                 enforce_polarity: Optional[bool] = False, decay: float = 0.0, parent_feature=None,
                 sparse: Optional[bool] = False, batch_size: int = 1, **kwargs) -> None:
        from ..learning.MCC_learning import MSTDP, MSTDPET, NoOp, PostPre
        assert isinstance(name, str), f"Feature {name}'s name should be of type str"
        assert value is None or isinstance(value, (torch.Tensor, float, int)), (
            f"Feature {name} should be of type float, int, or torch.Tensor, not {type(value)}")
        assert norm is None or isinstance(norm, (torch.Tensor, float, int)), (
            f"Feature {name}'s norm should be of type float, int, or torch.Tensor, not {type(norm)}")
        assert learning_rule is None or learning_rule in (NoOp, PostPre, MSTDP, MSTDPET), (
            f"Feature {name}'s learning_rule should be of type bindsnet.LearningRule not {type(learning_rule)}")
        assert nu is None or isinstance(nu, (list, tuple)), (
            f"Feature {name}'s nu should be of type list or tuple, not {type(nu)}")
        assert reduction is None or callable(reduction), f"Feature {name}'s reduction should be callable"
        assert decay is None or isinstance(decay, float), f"Feature {name}'s decay should be of type float"
        if sparse or parent_feature is not None or enforce_polarity:
            raise NotImplementedError("bindsnet_amd: sparse / linked / polarity-enforcing features are outside "
                                      "the accelerated path")
        self.name, self.value = name, value
        self.range = [-1.0, 1.0] if range is None else range
        self.clamp_frequency, self.norm, self.learning_rule = clamp_frequency, norm, learning_rule
        self.nu, self.reduction, self.decay = nu, reduction, decay
        self.parent_feature, self.sparse, self.batch_size, self.kwargs = parent_feature, sparse, batch_size, kwargs
        self.is_primed = False
        r = self.range
        assert isinstance(r, (list, tuple)) and len(r) == 2, f"Invalid range for feature {name}"
        lo_hi_ok = (r[0] < r[1]).all() if isinstance(r[0], torch.Tensor) or isinstance(r[1], torch.Tensor) else r[0] < r[1]
        assert lo_hi_ok, f"Invalid range for feature {name}: the min value is larger than the max value"
        if value is None:
            return
        if isinstance(value, torch.Tensor):
            assert (value >= r[0]).all() and (value <= r[1]).all(), (
                f"Feature out of range for {name}: Features values not in [{r[0]}, {r[1]}]")
            if value.dtype != value_dtype:
                warnings.warn(f"Provided value has data type {value.dtype} but parameter w_dtype is {value_dtype}")
                self.value = value.to(dtype=value_dtype)
        else:
            assert r[0] <= value <= r[1], f"Feature out of range for {name}"

    def prime_feature(self, connection, device, **kwargs) -> None:
        """Reference: topology_features.py:173-240 -- shape checks, Parameter-isation, rule construction."""
        from ..learning.MCC_learning import NoOp
        if self.is_primed:
            return
        self.is_primed = True
        if isinstance(self.value, torch.Tensor):
            assert tuple(self.value.shape) == (connection.source.n, connection.target.n)
        if self.norm is not None and isinstance(self.norm, torch.Tensor):
            assert self.norm.shape[0] == connection.target.n
        if self.value is None:
            self.value = self.initialize_value()
        if isinstance(self.value, (int, float)):
            self.value = torch.Tensor([self.value])
        self.value = Parameter(self.value, requires_grad=False).to(device)
        rule = NoOp if self.learning_rule is None else self.learning_rule
        self.learning_rule = rule(connection=connection, feature_value=self.value, range=self.range, nu=self.nu,
                                  reduction=self.reduction, decay=self.decay, **kwargs)
        del self.nu, self.reduction, self.decay, self.range

    def update(self, **kwargs) -> None:
        self.learning_rule.update(**kwargs)

    def normalize(self) -> None:
        """Reference: topology_features.py:250-266 (signed column sums) -> snn_normalize(use_abs=0); a float16 / bfloat16 value ->
        snn_normalize_h16 (the reference's three roundings: csrc/snn_half.hpp)."""
        if self.norm is None:
            return
        from .. import ops
        norm = self.norm if isinstance(self.norm, torch.Tensor) and self.norm.numel() > 1 else float(self.norm)
        ops.normalize(self.value.data, norm, use_abs=False)

    def reset_state_variables(self) -> None:
        if self.learning_rule:
            self.learning_rule.reset_state_variables()

    def to(self, device):
        """Move the value (the reference forgets to: SURVEY.md finding 8)."""
        if isinstance(self.value, torch.Tensor) and self.value.device != torch.device(device):
            self.value = Parameter(self.value.data.to(device), requires_grad=False)
            if hasattr(self.learning_rule, "feature_value"):
                self.learning_rule.feature_value = self.value
        if isinstance(self.value, torch.Tensor) and hasattr(self.learning_rule, "_move_rings") and not isinstance(self.learning_rule, type):
            self.learning_rule._move_rings(self.value.device)        # the rings of average_update live beside the value
        return self


class Weight(AbstractFeature):
    """Per-synapse scalar gain (reference: topology_features.py:575-671).  norm_frequency="sample": normalised at the end of run();
    "time step": behind every compute() of its connection instead (float32; the generic plan, snn_conn_desc.norm_step)."""

    def __init__(self, name: str, value=None, value_dtype: torch.dtype = torch.float32,
                 range: Optional[Sequence[float]] = None, norm=None, norm_frequency: Optional[str] = "sample",
                 learning_rule=None, nu: Optional[Union[list, tuple]] = None, reduction=None,
                 enforce_polarity: Optional[bool] = False, decay: float = 0.0, sparse: Optional[bool] = False,
                 batch_size: int = 1) -> None:
        if norm_frequency not in ("sample", "time step"):
            raise NotImplementedError(f"bindsnet_amd: norm_frequency={norm_frequency!r} is outside the accelerated path "
                                      "('sample' and 'time step' are supported)")
        if norm_frequency == "time step" and value_dtype in (torch.float16, torch.bfloat16):      # (a given value is cast to value_dtype)
            raise NotImplementedError(f"bindsnet_amd: norm_frequency='time step' on a {value_dtype} Weight is not supported (float32 is)")
        self.norm_frequency, self.enforce_polarity = norm_frequency, enforce_polarity
        if value_dtype in (torch.float16, torch.bfloat16) and isinstance(norm, torch.Tensor):
            raise NotImplementedError(f"bindsnet_amd: tensor norms are not supported on a {value_dtype} Weight")
        super().__init__(name=name, value=value, value_dtype=value_dtype,
                         range=[-torch.inf, +torch.inf] if range is None else range, norm=norm,
                         learning_rule=learning_rule, nu=nu, reduction=reduction, decay=decay, sparse=sparse,
                         batch_size=batch_size, enforce_polarity=enforce_polarity)

    def prime_feature(self, connection, device, **kwargs) -> None:
        if self.value is None:
            self.initialize_value = lambda: torch.rand(connection.source.n, connection.target.n)
        super().prime_feature(connection, device, enforce_polarity=self.enforce_polarity, **kwargs)

    def reset_state_variables(self) -> None:
        pass

    def _norm_step(self) -> bool:
        """norm_frequency="time step" with a norm: the value is normalised behind every compute() of its connection, learning or
        not, and by nothing else (reference: topology_features.py:641-643, :663-671)."""
        return self.norm_frequency == "time step" and self.norm is not None

    def normalize(self) -> None:
        """Reference: topology_features.py:663-671 -- called from outside compute() (Network.run's end, connection.normalize()) this
        normalises a "sample" Weight only."""
        if self.norm_frequency == "sample":
            super().normalize()

    def compute(self, conn_spikes):
        raise NotImplementedError("Weight.compute is fused into MulticompartmentConnection.compute on the device")


def _tensor_only(feature, value) -> None:
    """The reference casts every given value with `value.dtype` (topology_features.py:133, :146-153): a python scalar fails
    there with AttributeError, after the range assertions."""
    if value is not None and not isinstance(value, torch.Tensor):
        raise AttributeError(f"'{type(value).__name__}' object has no attribute 'dtype'")


class Probability(AbstractFeature):
    """Bernoulli gate per synapse and timestep (reference: topology_features.py:365-464): one torch.bernoulli(value) per
    compute() call from the global CPU generator, shared by the samples of the batch."""

    def __init__(self, name: str, value=None, value_dtype: torch.dtype = torch.float32,
                 range: Optional[Sequence[float]] = None, norm=None, learning_rule=None,
                 nu: Optional[Union[list, tuple]] = None, reduction=None, decay: float = 0.0, parent_feature=None,
                 sparse: Optional[bool] = False, batch_size: int = 1) -> None:
        from ..learning.MCC_learning import NoOp
        if learning_rule is not None and learning_rule is not NoOp:
            raise NotImplementedError("bindsnet_amd: a learning rule on a Probability is outside the accelerated path "
                                      "(rules are accepted on a Weight)")
        r = [0, 1] if range is None else range
        if isinstance(r, (list, tuple)) and len(r) == 2:                  # topology_features.py:445-464
            if isinstance(r[0], torch.Tensor):
                assert (r[0] >= 0).all(), f"Invalid range for feature {name}: a min value is less than 0"
            elif isinstance(r[0], (float, int)):
                assert r[0] >= 0, f"Invalid range for feature {name}: the min value is less than 0"
            else:
                assert False, f"Invalid range for feature {name}: the min value must be of type torch.Tensor, float, or int"
        super().__init__(name=name, value=value, value_dtype=value_dtype, range=r, norm=norm, learning_rule=learning_rule,
                         nu=nu, reduction=reduction, decay=decay, parent_feature=parent_feature, sparse=sparse,
                         batch_size=batch_size)
        _tensor_only(self, value)

    def prime_feature(self, connection, device, **kwargs) -> None:
        if self.value is None:
            self.initialize_value = lambda: torch.clamp(torch.rand(connection.source.n, connection.target.n, device=device),
                                                        self.range[0], self.range[1])
        super().prime_feature(connection, device, **kwargs)

    def reset_state_variables(self) -> None:
        pass

    def compute(self, conn_spikes):
        return conn_spikes * torch.bernoulli(self.value)


class Mask(AbstractFeature):
    """Boolean gate per synapse (reference: topology_features.py:467-549)."""

    def __init__(self, name: str, value=None, sparse: Optional[bool] = False, batch_size: int = 1) -> None:
        if isinstance(value, torch.Tensor):
            assert value.dtype == torch.bool, "Mask must be of type bool, not {}".format(value.dtype)
        elif value is not None:
            # (the reference formats its assertion message with value.dtype: any other scalar fails with AttributeError)
            assert isinstance(value, bool), "Mask must be of type bool, not {}".format(value.dtype)
            value = torch.tensor(value)
        super().__init__(name=name, value=value, value_dtype=torch.bool, sparse=sparse, batch_size=batch_size)
        self.name, self.value = name, value

    def prime_feature(self, connection, device, **kwargs) -> None:
        from ..learning.MCC_learning import NoOp
        if self.is_primed:
            return
        self.is_primed = True
        if self.value is None:
            self.value = (torch.rand(connection.source.n, connection.target.n) > 0.99).to(device=device)
        self.value = Parameter(self.value, requires_grad=False).to(device)
        if self.value.dim() > 1:                                          # (a scalar is a valid shape: :347-362)
            assert tuple(self.value.shape) == (connection.source.n, connection.target.n), (
                f"Feature {self.name} has an incorrect shape of {self.value.shape}. Should be of shape "
                f"{(connection.source.n, connection.target.n)}")
        self.learning_rule = NoOp(connection=connection)

    def reset_state_variables(self) -> None:
        pass

    def compute(self, conn_spikes):
        return conn_spikes * self.value


class Bias(AbstractFeature):
    """Per-synapse additive term (reference: topology_features.py:674-721): added to EVERY synapse's signal, spike or not."""

    def __init__(self, name: str, value=None, value_dtype: torch.dtype = torch.float32,
                 range: Optional[Sequence[float]] = None, norm=None, sparse: Optional[bool] = False,
                 batch_size: int = 1) -> None:
        super().__init__(name=name, value=value, value_dtype=value_dtype,
                         range=[-torch.inf, +torch.inf] if range is None else range, norm=norm, sparse=sparse,
                         batch_size=batch_size)
        _tensor_only(self, value)

    def prime_feature(self, connection, device, **kwargs) -> None:
        if self.value is None:
            self.initialize_value = lambda: torch.rand(connection.source.n, connection.target.n)
        super().prime_feature(connection, device, **kwargs)

    def reset_state_variables(self) -> None:
        pass

    def compute(self, conn_spikes):
        return conn_spikes + self.value


class Intensity(AbstractFeature):
    """Per-synapse scale without a rule (reference: topology_features.py:724-769)."""

    def __init__(self, name: str, value=None, value_dtype: torch.dtype = torch.float32,
                 range: Optional[Sequence[float]] = None, sparse: Optional[bool] = False, batch_size: int = 1) -> None:
        super().__init__(name=name, value=value, value_dtype=value_dtype, range=range, sparse=sparse, batch_size=batch_size)
        _tensor_only(self, value)

    def prime_feature(self, connection, device, **kwargs) -> None:
        if self.value is None:
            self.initialize_value = lambda: torch.clamp(
                torch.sign(torch.randint(-1, +2, (connection.source.n, connection.target.n))), self.range[0], self.range[1])
        super().prime_feature(connection, device, **kwargs)

    def reset_state_variables(self) -> None:
        pass

    def compute(self, conn_spikes):
        return conn_spikes * self.value


def _outside(name):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"bindsnet_amd: the {name} feature is outside the accelerated path")
    return type(name, (AbstractFeature,), {"__init__": __init__, "__doc__": f"Reference feature `{name}`: not provided."})


Degradation, MeanField = _outside("Degradation"), _outside("MeanField")
AdaptationBaseSynapsHistory, AdaptationBaseOtherSynaps = _outside("AdaptationBaseSynapsHistory"), _outside("AdaptationBaseOtherSynaps")
