"""The per-synapse update kernels' arithmetic on the HOST: tests/hostcheck/synparams_host.hip compiles the __host__ __device__ bodies of
csrc/snn_synparams.hpp with hipcc (no GPU needed) and drives them element by element, as the kernels' threads do
(tests/synparams_hostlib.py).

  * every op-level fixture case of tests/synparams_cases.py (reference-generated): w after every update() call and after normalize(),
    bit for bit;
  * against torch's own expressions on random shapes, S = 1 and N = 1 among them, with every constant in every shape that
    broadcasts against [S, N] -- [S, N], [N], [1, N], [S, 1], one element -- and one bound a tensor while the other is a float."""
import itertools
import os
import shutil

import numpy as np
import pytest
import torch

import synparams_cases as SC
from synparams_hostlib import HIPCC, HostLib
from test_synparams_host import bits, gold


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    return HostLib(tmp_path_factory.mktemp("hostcheck"))


def _t(a):
    return torch.from_numpy(np.array(a, np.float32)) if isinstance(a, np.ndarray) else a


DECAY_E = float(torch.exp(-torch.tensor(1.0) / torch.tensor(25.0)))     # tc_e_trace = 25


@pytest.mark.parametrize("case", list(SC.OP_CASES))
def test_bodies_reproduce_reference_fixture(host, case):
    c = SC.OP_CASES[case]
    g = gold(f"synparams_op_{c['rule']}.npz")
    k = SC.constants(case)
    nu0, nu1, wmin, wmax = _t(k["nu"][0]), _t(k["nu"][1]), _t(k["wmin"]), _t(k["wmax"])
    W = torch.from_numpy(SC.w0(case).copy())
    W = torch.clamp(W, torch.as_tensor(wmin), torch.as_tensor(wmax)).contiguous()          # topology.py:309-318: a given w is clamped to the bounds
    B = c["B"]
    states = SC.op_states(case)
    e_trace = torch.zeros(SC.S, SC.N)
    zs, zt = torch.zeros(B, SC.S), torch.zeros(B, SC.N)
    for i, (ss, xs, st, xt, reward) in enumerate(states):
        ss, xs, st, xt = (torch.from_numpy(a) for a in (ss, xs, st, xt))
        if c["rule"] == "PostPre":
            host.update("postpre", W, ss, xs, st, xt, nu0, nu1, wmin=wmin, wmax=wmax)
        elif c["rule"] == "Hebbian":
            host.update("hebbian", W, ss, xs, st, xt, nu0, nu1, wmin=wmin, wmax=wmax)
        elif c["rule"] == "WeightDependentPostPre":
            host.update("wdpostpre", W, ss, xs, st, xt, nu0, nu1, wmin=wmin, wmax=wmax)
        else:
            prev = states[i - 1] if i else None
            pp = torch.from_numpy(g[f"{case}/p_plus{i - 1}"]) if i else zs
            pm = torch.from_numpy(g[f"{case}/p_minus{i - 1}"]) if i else zt
            sp = torch.from_numpy(prev[0]) if i else zs.bool()
            tp = torch.from_numpy(prev[2]) if i else zt.bool()
            if c["rule"] == "MSTDP":
                host.update("mstdp", W, sp, pp.reshape(B, -1), tp, pm.reshape(B, -1), nu0, wmin=wmin, wmax=wmax, reward=reward)
            else:
                host.mstdpet(W, e_trace, pp.reshape(-1), pm.reshape(-1), sp.reshape(-1), tp.reshape(-1), reward, nu0, 1.0, DECAY_E, 25.0,
                             wmin=wmin, wmax=wmax)
                assert np.array_equal(bits(e_trace.numpy()), bits(g[f"{case}/eligibility_trace{i}"])), f"{case}: eligibility_trace after call {i}"
        want = g[f"{case}/w{i}"]
        assert np.array_equal(bits(W.numpy()), bits(want)), f"{case}: w after call {i} differs in {(bits(W.numpy()) != bits(want)).sum()} elements"
    norm = np.asarray(k["norm"])
    if norm.ndim == 1 or norm.shape[0] == 1:
        host.normalize(W, torch.from_numpy(norm.copy()), use_abs=True)
        assert np.array_equal(bits(W.numpy()), bits(g[f"{case}/w_norm"])), f"{case}: w after normalize()"


SHAPES = ("SN", "N", "1N", "S1", "1", "float")


def _const(rng, code, S, N, lo, hi):
    if code == "float":
        return float(np.float32(lo + (hi - lo) * rng.random()))
    shape = {"SN": (S, N), "N": (N,), "1N": (1, N), "S1": (S, 1), "1": (1,)}[code]
    return torch.from_numpy((lo + (hi - lo) * rng.random(shape)).astype(np.float32))


def torch_update(mode, W, ss, xs, st, xt, nu0, nu1, wmin, wmax, reward=0.0):
    """The reference's statements (learning.py) on [B, S] / [B, N] factors, batch-summed by torch."""
    B = ss.shape[0]
    red = (lambda t: t.squeeze(0)) if B == 1 else (lambda t: torch.sum(t, dim=0))
    ssf, stf = ss.float(), st.float()
    any0 = bool(torch.as_tensor(nu0).any())
    any1 = bool(torch.as_tensor(nu1).any())
    W = W.clone()
    if mode == "postpre":
        if any0:
            W -= red(torch.bmm(ssf.unsqueeze(2), xt.unsqueeze(1) * nu0))
        if any1:
            W += red(torch.bmm(xs.unsqueeze(2), stf.unsqueeze(1) * nu1))
    elif mode == "mstdp":
        elig = torch.bmm(xs.unsqueeze(2), stf.unsqueeze(1)) + torch.bmm(ssf.unsqueeze(2), xt.unsqueeze(1))
        W += nu0 * red(reward * elig)
    else:
        u1 = red(torch.bmm(ssf.unsqueeze(2), xt.unsqueeze(1)))
        u2 = red(torch.bmm(xs.unsqueeze(2), stf.unsqueeze(1)))
        if mode == "hebbian":
            W += nu0 * u1
            W += nu1 * u2
        else:
            update = 0
            if any0:
                update = update - nu0 * u1 * (W - wmin)
            if any1:
                update = update + nu1 * u2 * (wmax - W)
            W += update
    return torch.clamp(W, torch.as_tensor(wmin), torch.as_tensor(wmax))


@pytest.mark.parametrize("mode", ["postpre", "hebbian", "wdpostpre", "mstdp"])
def test_bodies_equal_torch_on_every_stride_combination(host, mode):
    rng = np.random.default_rng(len(mode))
    tried = 0
    for (S, N), B in itertools.product(((1, 1), (1, 7), (1, 9), (9, 1), (5, 33), (19, 40)), (1, 3, 33)):
        if S * N < 8 and B > 1:
            continue                              # (fewer than 8 weights: ATen sums the batch in another order than the kernels' accumulator, scalar or not)
        combos = list(itertools.product(SHAPES, repeat=2))
        for a, b in combos:                       # a: shape of the rates, b: shape of the lower bound; the upper bound takes the next shape
            if mode == "postpre" and a in ("SN", "S1") and S > 1:
                continue                          # (learning.py:401-402: fails in the reference)
            c = SHAPES[(SHAPES.index(b) + 1) % len(SHAPES)]
            nu0, nu1 = _const(rng, a, S, N, -0.3, 0.3), _const(rng, a, S, N, 0.0, 0.3)
            wmin, wmax = _const(rng, b, S, N, 0.1, 0.4), _const(rng, c, S, N, 0.6, 0.9)
            W = torch.from_numpy(rng.random((S, N)).astype(np.float32))
            ss, st = torch.from_numpy(rng.random((B, S)) < 0.4), torch.from_numpy(rng.random((B, N)) < 0.4)
            xs, xt = torch.from_numpy(rng.random((B, S)).astype(np.float32)), torch.from_numpy(rng.random((B, N)).astype(np.float32))
            want = torch_update(mode, W, ss, xs, st, xt, nu0, nu1, wmin, wmax, reward=0.7)
            got = W.clone()
            host.update(mode, got, ss, xs, st, xt, nu0, nu1, wmin=wmin, wmax=wmax, reward=0.7)
            assert np.array_equal(bits(got.numpy()), bits(want.numpy())), (mode, S, N, B, a, b, c)
            tried += 1
    assert tried > 300


def test_normalize_body_divides(host):
    rng = np.random.default_rng(5)
    differ = 0
    for S, N in ((1, 1), (7, 1), (1, 9), (37, 29), (64, 130)):
        W = torch.from_numpy((rng.random((S, N)) - 0.3).astype(np.float32))
        W[:, 0] = 0.0                                 # a zero column: the guard
        norm = torch.from_numpy((1.0 + rng.random(N) * 20).astype(np.float32))
        for use_abs in (True, False):
            colsum = (W.abs() if use_abs else W).sum(0).unsqueeze(0)
            colsum[colsum == 0] = 1.0
            want = W * (norm / colsum)
            got = W.clone()
            host.normalize(got, norm, use_abs)
            assert np.array_equal(bits(got.numpy()), bits(want.numpy())), (S, N, use_abs)
            differ += int((bits((W * (norm * (1.0 / colsum))).numpy()) != bits(want.numpy())).sum())
    assert differ > 0, "norm / colsum never differed from norm * (1 / colsum): the test shows nothing"
