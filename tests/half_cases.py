"""The float16 / bfloat16 Weight fixture cases (tests/golden/make_golden_half.py), written once for both implementations:
`build(ns, name)` constructs a case's DiehlAndCook2015 from a namespace of classes -- the reference's (the generator) or this
package's (the tests) -- and `run_case` drives it and records, after every one of 3 consecutive inputs (reset_state_variables()
between them, so the X -> Ae weights are normalised between inputs): the Ae and Ai rasters, v / refrac_count of both layers, theta,
both traces, the learned X -> Ae `value` as raw 16-bit patterns, and the global generator's state (one_spike draws from it).

(a) 784 -> 40, batch 4, 60 steps, input density 0.12, float16: PostPre with the batch sum, norm 78.4, range [0, 1]
(b) (a) with bfloat16
(c) a [1, 10, 10] input -> 33 neurons, batch 1, float16: rows of an odd N are only 2-byte aligned, and the batch reduction has one term
(d) (c) with bfloat16 at dt = 0.5
(e) (a) with network.train(False)"""
import hashlib
from types import SimpleNamespace

import numpy as np
import torch

from dt_cases import run_time

N_IN = 3
CASES = {
    "a": dict(n_inpt=784, shape=None, N=40, B=4, T=60, density=0.12, dtype="float16", norm=78.4, nu=(1e-4, 1e-2), dt=1.0, train=True, seed=0),
    "c": dict(n_inpt=100, shape=(1, 10, 10), N=33, B=1, T=60, density=0.5, dtype="float16", norm=20.0, nu=(1e-2, 5e-2), dt=1.0, train=True,
              seed=1),
}
CASES["b"] = dict(CASES["a"], dtype="bfloat16")
CASES["d"] = dict(CASES["c"], dtype="bfloat16", dt=0.5)
CASES["e"] = dict(CASES["a"], train=False)
TRAINING = tuple(k for k in sorted(CASES) if CASES[k]["train"])


def dtype_of(name):
    return getattr(torch, CASES[name]["dtype"])


def ns_from(models, monitors):
    return SimpleNamespace(DiehlAndCook2015=models.DiehlAndCook2015, Monitor=monitors.Monitor)


def build(ns, name, **over):
    """The case's network: the model's own constructor after torch.manual_seed(seed), as batch_eth_mnist.py calls it."""
    c = dict(CASES[name], **over)
    torch.manual_seed(c["seed"])
    # (reduction stays None: it resolves to torch.sum, because the layers do not belong to a network yet when the rule is made,
    #  MCC_learning.py:75-81 -- also at batch 1, where the sum over the one sample is that sample's term)
    net = ns.DiehlAndCook2015(n_inpt=c["n_inpt"], n_neurons=c["N"], batch_size=c["B"], dt=c["dt"], norm=c["norm"], nu=c["nu"],
                              inpt_shape=c["shape"], w_dtype=getattr(torch, c["dtype"]))
    if not c["train"]:
        net.train(False)
    return net


def inputs(name, r):
    """Input `r` of a case: [T, B, *input shape] uint8 from numpy's generator (the same draws everywhere)."""
    c = CASES[name]
    rng = np.random.default_rng(1000 * c["seed"] + r + 11)
    shape = (c["n_inpt"],) if c["shape"] is None else c["shape"]
    return (rng.random((c["T"], c["B"], *shape)) < c["density"]).astype(np.uint8)


def value_of(net):
    return net.connections[("X", "Ae")].pipeline[0].value


def bits16(t):
    """A float16 / bfloat16 tensor's raw patterns as a uint16 array."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def snapshot(net, ras_e, ras_i):
    X, Ae, Ai = net.layers["X"], net.layers["Ae"], net.layers["Ai"]
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).copy()      # noqa: E731
    return dict(sE=np.asarray(ras_e, np.uint8), sI=np.asarray(ras_i, np.uint8), vE=f(Ae.v), vI=f(Ai.v), theta=f(Ae.theta),
                refracE=f(Ae.refrac_count), refracI=f(Ai.refrac_count), xX=f(X.x), xE=f(Ae.x), value=bits16(value_of(net)),
                rng=torch.get_rng_state().numpy().copy())


def run_case(net, name, monitor_cls, device=None, first=0, count=None, pieces=1):
    """Run inputs [first, first + count) of the case; one snapshot per input.  pieces > 1: every input as that many run() calls."""
    c = CASES[name]
    out = []
    count = N_IN - first if count is None else count
    for r in range(first, first + count):
        x = torch.from_numpy(inputs(name, r))
        if device is not None:
            x = x.to(device)
        step = c["T"] // pieces
        ras_e, ras_i = [], []
        for p in range(pieces):
            mons = {"Ae_s": monitor_cls(net.layers["Ae"], ["s"], time=step), "Ai_s": monitor_cls(net.layers["Ai"], ["s"], time=step)}
            for k, m in mons.items():
                net.add_monitor(m, name=k)
            net.run({"X": x[p * step:(p + 1) * step]}, time=run_time(step, c["dt"]))
            ras_e.append(mons["Ae_s"].get("s").cpu().numpy().reshape(step, c["B"], -1).astype(np.uint8))
            ras_i.append(mons["Ai_s"].get("s").cpu().numpy().reshape(step, c["B"], -1).astype(np.uint8))
            for k in mons:
                del net.monitors[k]
        out.append(snapshot(net, np.concatenate(ras_e), np.concatenate(ras_i)))
        net.reset_state_variables()
    return out


# ---- the kernel-level sweeps (tests/test_half_hostcheck.py on the host bodies, tests/test_gpu_half.py on the device) -------------
# The torch expressions below are the reference's own statements on CPU tensors (topology.py:437-479 with topology_features.py:633-645,
# MCC_learning.py:224-302 + :86-110, topology_features.py:264-266); every comparison against them is on raw bit patterns.
SWEEP_N, SWEEP_NIN, SWEEP_B, SWEEP_DENSITY = (1, 7, 33, 40, 400), (17, 100, 784), (1, 3, 33), (0.0, 0.02, 0.3, 1.0)
# (nu0, nu1, decay argument of the rule, (min, max), dt): both halves; each half alone; a decay; bounds that neither dtype represents
RULES = {
    "both": (1e-2, 5e-2, 0.0, (None, None), 1.0),
    "nu0_zero": (0.0, 5e-2, 0.0, (None, None), 1.0),
    "nu1_zero": (1e-2, 0.0, 0.0, (None, None), 1.0),
    "decay": (1e-2, 5e-2, 0.01, (None, None), 1.0),
    "bounds_dt05": (2e-2, 8e-2, 0.01, (0.1, 0.3), 0.5),
}


def rand_weights(rng, Nin, N, dtype, scale=0.3):
    return torch.from_numpy((rng.random((Nin, N)) * scale).astype(np.float32)).to(dtype)


def rand_spikes(rng, B, n, density):
    return torch.from_numpy((rng.random((B, n)) < density).astype(np.uint8))


def ref_prop(W, s, before=None):
    """What the target's float32 current holds after the connection: zeros (or `before`) += compute(s)."""
    B, (Nin, N) = s.shape[0], W.shape
    conn_spikes = s.bool().view(B, Nin, 1).repeat(1, 1, N)
    out = torch.zeros(B, N) if before is None else before.clone()
    out += (W * conn_spikes).sum(1)
    return out


def ref_postpre(W, s_src, x_src, s_tgt, x_tgt, nu0, nu1, decay, lo, hi, dt, reduction=None):
    """MCC PostPre's statements on a clone of W; reduction None: the rule's default (squeeze at batch 1, else sum)."""
    B = s_src.shape[0]
    W = W.clone()
    nu = torch.zeros(2, dtype=torch.float)
    nu[0], nu[1] = nu0, nu1
    reduction = reduction or (torch.squeeze if B == 1 else torch.sum)
    factor = 1.0 - decay if decay else 1.0
    if nu[0]:
        source_s = s_src.view(B, -1).unsqueeze(2).float()
        target_x = x_tgt.view(B, -1).unsqueeze(1) * nu[0]
        W -= reduction(torch.bmm(source_s, target_x), dim=0) * dt
    if nu[1]:
        target_s = s_tgt.view(B, -1).unsqueeze(1).float() * nu[1]
        source_x = x_src.view(B, -1).unsqueeze(2)
        W += reduction(torch.bmm(source_x, target_s), dim=0) * dt
    if factor:
        W *= factor
    if lo is not None or hi is not None:
        W.clamp_(lo, hi)
    return W, float(nu[0]), float(nu[1]), factor


def ref_normalize(W, norm):
    W = W.clone()
    abs_sum = W.sum(0).unsqueeze(0)
    abs_sum[abs_sum == 0] = 1.0
    W *= norm / abs_sum
    return W
