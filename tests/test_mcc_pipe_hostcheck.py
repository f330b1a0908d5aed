"""The feature-pipeline kernels' arithmetic on the HOST: tests/hostcheck/mccpipe_host.hip compiles the __host__ __device__ term
program and draw-to-bit conversion of csrc/snn_mccpipe.hpp with hipcc (no GPU needed) and drives them with the ordered-sum
accumulators of csrc/snn_order.hpp, synapse by synapse, as the kernels' threads do.

  * the summed terms against torch's own expression (repeat, the features' multiplies and adds in order, sum(1)) on the shapes and
    pipelines of tests/mcc_pipe_cases.py, bit for bit, with signed zeros in the values;
  * the bit mask against torch.bernoulli from the same generator state for S*N in {1, 623, 624, 625, 1255}, from a fresh block,
    from the middle of one and across its end; the generator position afterwards is torch's."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mcc_pipe_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KIND = {"P": 1, "M": 2, "W": 3, "I": 3, "B": 4}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libmccpipehost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "mccpipe_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.hostcheck_mcc_prop.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.hostcheck_mcc_prop.restype = None
    lib.hostcheck_mcc_bernoulli.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.hostcheck_mcc_bernoulli.restype = None
    return lib


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _pack(hits):
    """bool [S, N] -> the device's uint32 [S, ceil(N/32)] layout."""
    S, N = hits.shape
    padded = np.zeros((S, (N + 31) // 32 * 32), np.uint8)
    padded[:, :N] = hits
    return np.ascontiguousarray(np.packbits(padded.reshape(S, -1, 32), axis=2, bitorder="little").view(np.uint32).reshape(S, -1))


def _torch_sum(pipe, vals, s):
    B, S = s.shape
    N = next(v for v in vals if v.ndim == 2).shape[1]
    x = torch.from_numpy(s).view(B, S, 1).repeat(1, 1, N)
    for ch, v in zip(pipe, vals):
        t = torch.from_numpy(v)
        x = t * x if ch == "W" else x + t if ch == "B" else x * t
    return x.sum(1).numpy()


SHAPES = sorted({(c["pipe"], c["S"], c["N"], c["B"]) for c in PC.CASES.values()}) + [("PW", 20, 20, 3), ("PMWB", 1, 1, 1), ("IWB", 257, 65, 2)]


@pytest.mark.parametrize("pipe,S,N,B", SHAPES)
def test_term_program_and_ordered_sum_equal_torch(host, pipe, S, N, B):
    rng = np.random.default_rng(S * 1000 + N)
    s = (rng.random((B, S)) < 0.3).astype(np.uint8)
    vals, dev_vals, keep = [], [], []
    for ch in pipe:
        if ch == "P":                                   # (the draw itself is checked below: here a given outcome)
            hits = rng.random((S, N)) < 0.6
            vals.append(hits.astype(np.float32))
            dev_vals.append(_pack(hits))
        elif ch == "M":
            m = rng.random((S, N)) < 0.7
            vals.append(m)
            dev_vals.append(m.astype(np.uint8))
        else:
            v = ((rng.random((S, N), dtype=np.float32) - np.float32(0.3)) * np.float32(2.0)).astype(np.float32)
            v[rng.random((S, N)) < 0.05] = -0.0         # signed zeros go through real multiplies
            vals.append(v)
            dev_vals.append(v)
    kinds = np.array([KIND[ch] for ch in pipe], np.int32)
    ptrs = (C.c_void_p * len(pipe))(*[v.ctypes.data for v in dev_vals])
    scalars = np.zeros(len(pipe), np.int32)
    out = np.zeros((B, N), np.float32)
    host.hostcheck_mcc_prop(len(pipe), _p(kinds), C.cast(ptrs, C.c_void_p), _p(scalars), _p(s), B, S, N, _p(out))
    want = _torch_sum(pipe, vals, s)
    assert want.dtype == np.float32
    bad = np.flatnonzero(out.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert bad.size == 0, f"{pipe} [{B},{S},{N}]: {bad.size} of {out.size} sums differ from torch (first {bad[:5]})"
    assert np.abs(want).sum() > 0


def test_scalar_operands(host):
    S, N, B = 40, 33, 2
    rng = np.random.default_rng(1)
    s = (rng.random((B, S)) < 0.4).astype(np.uint8)
    w = rng.random((S, N), dtype=np.float32)
    g, b = np.array([0.75], np.float32), np.array([0.015625], np.float32)
    kinds, scalars = np.array([3, 3, 4], np.int32), np.array([0, 1, 1], np.int32)
    ptrs = (C.c_void_p * 3)(w.ctypes.data, g.ctypes.data, b.ctypes.data)
    out = np.zeros((B, N), np.float32)
    host.hostcheck_mcc_prop(3, _p(kinds), C.cast(ptrs, C.c_void_p), _p(scalars), _p(s), B, S, N, _p(out))
    x = torch.from_numpy(s).view(B, S, 1).repeat(1, 1, N)
    want = (((torch.from_numpy(w) * x) * torch.from_numpy(g)) + torch.from_numpy(b)).sum(1).numpy()
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("S,N", [(1, 1), (7, 89), (16, 39), (25, 25), (5, 251)])          # S*N = 1, 623, 624, 625, 1255
@pytest.mark.parametrize("warm", [0, 5, 620])
def test_bit_mask_equals_torch_bernoulli(host, S, N, warm):
    from bindsnet_amd import rng
    torch.manual_seed(100 + S)
    if warm:
        torch.rand(warm)
    p = torch.rand(S, N)                                # (also moves the generator into a block)
    st = torch.get_rng_state()
    img = rng.torch_state_to_words(st)
    mt, pos = img[:624].view(np.uint32).copy(), np.array([int(img[624])], np.int32)
    bits = np.full((S, (N + 31) // 32), 0xFFFFFFFF, np.uint32)
    host.hostcheck_mcc_bernoulli(_p(mt), _p(pos), _p(p.numpy()), 0, S, N, _p(bits))
    want = torch.bernoulli(p).numpy() != 0
    assert np.array_equal(bits, _pack(want)), f"S*N = {S * N}: mask differs from torch.bernoulli"
    img2 = img.copy()
    img2[:624], img2[624] = mt.view(np.int32), int(pos[0])
    after = torch.get_rng_state()
    torch.set_rng_state(rng.words_to_torch_state(img2, st))
    a = torch.rand(5)
    torch.set_rng_state(after)
    assert torch.equal(a, torch.rand(5)), "the generator position afterwards is not torch's"
