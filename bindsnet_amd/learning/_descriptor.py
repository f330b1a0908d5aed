"""What the rules of learning.py and MCC_learning.py write into a snn_conn_desc (include/snnhip.h) for Network.run: the
parts both rule hierarchies share."""
import torch

from .. import _lib
from .._lib import dptr


class Rule(_lib.Touching):
    """What both rule trees say about a run before it starts (network/_preflight.py), each answer an exception or None."""

    _learns = True                     # whether the rule changes the weights: all but NoOp

    def _batch_refusal(self, B: int):
        """Why the rule cannot learn at batch size B."""

    def _syn_refusal(self):
        """What a rule with per-synapse constants cannot run: asked when the rule is built and before a run changes any state."""

    def _multi_device_refusal(self, mode: str, key):
        """The rule's reason against parallel.py's mode `mode`."""

    def _refusals(self, key, req):
        """Why the learning run `req` must not start with this rule on connection `key`: asked behind the connection's own."""
        yield self._batch_refusal(req.B)
        yield self._syn_refusal()


def accepts(connection, rule) -> bool:
    """True when the connection's family lists the rule's class (or one of its bases) by name in `_rules`."""
    return any(c.__name__ in getattr(connection, "_rules", ()) for c in type(rule).__mro__)


def is_vec(v) -> bool:
    """A constant given as a tensor of more than one element (a one-element tensor is a scalar, as for the node layers)."""
    return isinstance(v, torch.Tensor) and v.numel() > 1


def device_const(t, shape, dev):
    """A tensor constant as the *_pv kernels read it: (float32 contiguous tensor on `dev`, element strides against `shape`), 0 on
    every broadcast axis -- nothing is expanded.  A tensor that is not already there is copied once and kept on the tensor object,
    keyed by its in-place version; while run descriptors are built the tensor is noted, so an in-place edit rebuilds them.  What does
    not broadcast against `shape` raises torch's RuntimeError, as the reference's first update would."""
    from ..network import nodes as _nodes
    if _nodes._SCALARS is not None:
        _nodes._SCALARS.append((t, t._version))
    dev = torch.device(dev)
    if t.device == dev and t.dtype == torch.float32 and t.is_contiguous():
        c = t.detach()
    else:
        hit = getattr(t, "_snn_dev", None)
        if hit is None or hit[0] != t._version or hit[1].device != dev:
            hit = (t._version, t.detach().to(dev, torch.float32).contiguous())
            t._snn_dev = hit
        c = hit[1]
    e = c.expand(*shape)
    pad = len(shape) - c.dim()
    strides = tuple(0 if (k < pad or c.shape[k - pad] == 1) else e.stride(k) for k in range(len(shape)))
    return c, strides


def any_nonzero(t) -> bool:
    """`t.any()` of a rate tensor (learning.py:399), remembered on the tensor by its in-place version."""
    hit = getattr(t, "_snn_any", None)
    if hit is None or hit[0] != t._version:
        hit = (t._version, bool(t.any()))
        t._snn_any = hit
    return hit[1]


def all_finite(t) -> bool:
    hit = getattr(t, "_snn_finite", None)
    if hit is None or hit[0] != t._version:
        hit = (t._version, bool(torch.isfinite(t).all()))
        t._snn_finite = hit
    return hit[1]


def syn_params(S, N, dev, nu0, nu1, lo, hi):
    """The constants of one rule for the C ABI.  Each of nu0, nu1 (float or tensor) and lo, hi (None, float or tensor) goes either
    into its scalar argument or, as a tensor of more than one element, into the snn_synparams.  Returns (nu0, nu1, lo, hi, sp, keep):
    scalars (0.0 / None where a tensor stands), the _lib.SynParams or None when there is no tensor, the device tensors it points to."""
    vals = {"nu0": nu0, "nu1": nu1, "wmin": lo, "wmax": hi}
    if not any(is_vec(v) for v in vals.values()):
        return _scalar(nu0) or 0.0, _scalar(nu1) or 0.0, _bound(lo), _bound(hi), None, []
    sp, keep = _lib.SynParams(), []
    for name, v in vals.items():
        if not is_vec(v):
            continue
        c, (rs, cs) = device_const(v, (S, N), dev)
        keep.append(c)
        setattr(sp, name, c.data_ptr())
        setattr(sp, name + "_rs", rs)
        setattr(sp, name + "_cs", cs)
        if name in ("nu0", "nu1"):
            setattr(sp, name + "_any", int(any_nonzero(v)))
        vals[name] = None
    return _scalar(vals["nu0"]) or 0.0, _scalar(vals["nu1"]) or 0.0, _bound(vals["wmin"]), _bound(vals["wmax"]), sp, keep


def _scalar(v):
    if v is None:
        return None
    return float(v.reshape(()).item()) if isinstance(v, torch.Tensor) else float(v)


def _bound(v):
    v = _scalar(v)
    return None if v is None or v in (float("inf"), float("-inf")) else v


# The batch reductions a rule takes (learning.py:76-82, MCC_learning.py:75-81), with the name each goes by on the device (SNN_REDUCE_*,
# _lib.REDUCE); torch.squeeze is the sum path at batch size 1.
REDUCTIONS = ((torch.sum, "sum"), (torch.squeeze, "sum"), (torch.mean, "mean"), (torch.amax, "amax"), (torch.amin, "amin"))


def reduction_name(f) -> str:
    name = getattr(f, "__name__", None)
    return repr(f) if name is None else (f"torch.{name}" if getattr(torch, name, None) is f else name)


def check_reduction(rule) -> None:
    """Any callable but the five is refused by name."""
    if not any(rule.reduction is f for f, _ in REDUCTIONS):
        raise NotImplementedError(f"bindsnet_amd: reduction={reduction_name(rule.reduction)} is not supported: torch.sum, torch.squeeze "
                                  "(batch size 1), torch.mean, torch.amax and torch.amin are")


def reduce_of(rule, B: int) -> str:
    """The rule's batch reduction as the ops take it: "sum", "mean", "amax" or "amin".  At batch size 1 all five are the identity
    (x / 1.0f == x) and share the sum path, as torch.squeeze does."""
    check_reduction(rule)
    return "sum" if B == 1 else next(name for f, name in REDUCTIONS if rule.reduction is f)


def fill_update(d, rule, wdecay, dev=None, keep=None) -> None:
    """Clamp bounds, weight-decay factor (dense rules keep it in `weight_decay`, MCC rules in `decay`) and learning rates.  A rule
    that takes per-synapse constants (`_takes_syn`) hands tensors on: they go into d.syn, on `dev`."""
    d.wdecay = float(wdecay)
    if getattr(rule, "_takes_syn", False):
        lo, hi = rule._bounds(tensors=True)
        nu0, nu1 = rule._nu(0), rule._nu(1)
        if any(is_vec(v) for v in (nu0, nu1, lo, hi)):
            nu0, nu1, lo, hi, sp, kept = syn_params(rule.source.n, rule.target.n, dev, nu0, nu1, lo, hi)
            d.syn = sp
            if keep is not None:
                keep.extend(kept)
            d.has_min, d.wmin = int(lo is not None), lo or 0.0
            d.has_max, d.wmax = int(hi is not None), hi or 0.0
            d.nu0, d.nu1 = nu0, nu1
            return
    lo, hi = rule._bounds()
    d.has_min, d.wmin = int(lo is not None), lo or 0.0
    d.has_max, d.wmax = int(hi is not None), hi or 0.0
    d.nu0, d.nu1 = float(rule.nu[0]), float(rule.nu[1])


def reward(kwargs):
    """run(..., reward=...): a reward-modulated rule cannot run without it."""
    if "reward" not in kwargs:
        raise KeyError("reward")
    return kwargs["reward"]


def split_reward(r, dev):
    """(scalar reward, None), or (0.0, the per-sample rewards as a float32 vector on `dev`)."""
    if isinstance(r, torch.Tensor) and r.numel() > 1:
        return 0.0, r.to(dev, torch.float32).reshape(-1).contiguous()
    return float(r), None


def a_plus_minus(kwargs):
    a_plus, a_minus = kwargs.get("a_plus", 1.0), kwargs.get("a_minus", -1.0)
    if isinstance(a_plus, dict) or isinstance(a_minus, dict):
        raise NotImplementedError("bindsnet_amd: per-connection a_plus/a_minus dicts are not supported")
    return float(a_plus), float(a_minus)


def fill_mstdp(d, rule, kwargs, dev, keep) -> None:
    """Reward / a_plus / a_minus keyword arguments and the rule's device state (learning.py:1504-1574,
    MCC_learning.py:468-551)."""
    r = reward(kwargs)
    rule._ensure_state()
    d.reward, rv = split_reward(r, dev)
    if rv is not None:
        keep.append(rv)
        d.reward_vec = dptr(rv)
    d.rule = _lib.RULE_MSTDP
    d.a_plus, d.a_minus = a_plus_minus(kwargs)
    d.decay_plus, d.decay_minus = rule._decays()
    d.p_plus, d.p_minus = dptr(rule.p_plus), dptr(rule.p_minus)
    d.s_src_prev, d.s_tgt_prev = dptr(rule._s_src_prev), dptr(rule._s_tgt_prev)


def fill_mstdpet(d, rule, wdecay, kwargs, dev=None, keep=None) -> None:
    """MSTDPET's keyword arguments and device state (learning.py:2187-2248, MCC_learning.py:652-729)."""
    r = reward(kwargs)
    rule._ensure_state()
    fill_update(d, rule, wdecay, dev, keep)
    dp, dm, de = rule._decays()
    d.rule, d.reward = _lib.RULE_MSTDPET, float(r)
    d.a_plus, d.a_minus = float(kwargs.get("a_plus", 1.0)), float(kwargs.get("a_minus", -1.0))
    d.decay_plus, d.decay_minus, d.decay_e, d.tc_e = dp, dm, de, float(rule.tc_e_trace)
    d.p_plus, d.p_minus, d.e_trace = dptr(rule.p_plus), dptr(rule.p_minus), dptr(rule.eligibility_trace)
    d.s_src_prev, d.s_tgt_prev = dptr(rule._s_src_prev), dptr(rule._s_tgt_prev)
