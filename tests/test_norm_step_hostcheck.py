"""The fused propagate-and-normalise kernel's arithmetic on the HOST: tests/hostcheck/norm_step_host.hip compiles the __host__
__device__ text of csrc/snn_normstep.hpp with hipcc (no GPU needed) and drives it tile by tile, as the workgroups of
snn_prop_cascade_norm(_pv)_f32 do.

  * against the two-call arithmetic in torch -- the currents `0 (or out) + (W * s).sum(1)` from the old weights, then
    AbstractFeature.normalize's column scaling -- bit for bit in `out` and in W, over the shapes (Nin, N, B) below, spike densities
    0, 5 % and 100 %, accumulate 0 and 1, a scalar and a per-target norm, negative weights and a zero-sum column;
  * the fixture cases of tests/norm_step_cases.py (reference-generated) with this body in place of the host path's propagation of a
    single Weight: rasters, layer state, weights, rule state, bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import norm_step_cases as NC
from test_norm_step_host import ns, run_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SHAPES = ((1, 1, 1), (7, 31, 2), (70, 37, 3), (513, 96, 5), (784, 400, 32))      # (Nin, N, B)
EXTRA = ((40, 1, 3), (33, 5, 2), (64, 3, 1), (300, 70, 17))                        # one column, the 4..7 class, N < 4, more samples than a pass


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libnormstephost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "norm_step_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    lib.hostcheck_prop_norm.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_float, C.c_void_p]
    lib.hostcheck_prop_norm.restype = C.c_long
    return lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def operands(Nin, N, B, density, seed):
    """W of mixed sign with one all-zero column and (where there is room) one that sums to exactly 0; u8 spikes; a previous `out`."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.rand(Nin, N, generator=g) * 1.5 - 0.4).contiguous()
    if N >= 3:
        W[:, N // 2] = 0.0
    if N >= 4 and Nin >= 2:
        W[:, 1] = 0.0
        W[0, 1], W[Nin - 1, 1] = 0.5, -0.5
    s = (torch.rand(B, Nin, generator=g) < density).to(torch.uint8).contiguous()
    out0 = torch.randn(B, N, generator=g).contiguous()
    return W, s, out0


def two_calls(W, s, out0, accumulate, norm):
    """The reference's statements on the host: the signal from the old weights, then the in-place normalisation."""
    from bindsnet_amd.network import host_path
    B, (Nin, N) = s.shape[0], W.shape
    signal = W * s.float().reshape(B, Nin, 1).repeat(1, 1, N)
    W = W.clone()
    host_path._normalize_columns(W, norm, False)
    base = out0 if accumulate else torch.zeros(B, N)
    return base + host_path._sum(signal, 1), W


@pytest.mark.parametrize("shape", SHAPES + EXTRA)
@pytest.mark.parametrize("vector", (False, True))
def test_tiles_equal_the_two_calls(host, shape, vector):
    torch.set_num_threads(1)
    Nin, N, B = shape
    norm = torch.linspace(0.5, 2.5, N) if vector else 0.1 * Nin
    for density in (0.0, 0.05, 1.0):
        for accumulate in (0, 1):
            W, s, out0 = operands(Nin, N, B, density, 1000 * Nin + N + int(100 * density))
            want_out, want_W = two_calls(W, s, out0, accumulate, norm)
            out = out0.clone()
            lds = host.hostcheck_prop_norm(_p(W), _p(s), _p(out), B, Nin, N, accumulate, 0.0 if vector else norm, _p(norm if vector else None))
            assert 0 <= lds <= 150 * 1024, lds
            assert torch.equal(out, want_out), (shape, density, accumulate, int((out != want_out).sum()))
            assert torch.equal(W, want_W), (shape, density, accumulate, int((W != want_W).sum()))


@pytest.mark.parametrize("case", sorted(c for c in NC.CASES if NC.CASES[c].get("pipe") is None))
def test_fixture_case_with_the_kernel_body(host, monkeypatch, case):
    from bindsnet_amd.network import host_path
    calls = []

    def propagate(conn, s):
        feat = conn._weight()
        assert feat._norm_step()
        B, W = s.shape[0], feat.value.data
        out = torch.empty(B, conn.target.n)
        norm = feat.norm if isinstance(feat.norm, torch.Tensor) else float(feat.norm)
        vec = isinstance(norm, torch.Tensor)
        s8 = s.reshape(B, -1).to(torch.uint8).contiguous()
        assert host.hostcheck_prop_norm(_p(W), _p(s8), _p(out), B, W.shape[0], W.shape[1], 0, 0.0 if vec else norm,
                                        _p(norm.float().contiguous() if vec else None)) >= 0
        calls.append(1)
        return out.view(B, *conn.target.shape)

    monkeypatch.setattr(host_path, "_propagate_mcc", propagate)
    _, got = run_fixture(ns(), case)
    NC.assert_same(case, got, NC.gold(case, HERE), "kernel body on the host")
    c = NC.CASES[case]
    n_conn = 2 if c.get("graph") in ("two_layer", "two_inputs") else 1
    assert len(calls) == NC.INPUTS * c["T"] * n_conn          # exactly once per connection and timestep
