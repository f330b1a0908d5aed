"""The wide conv2d kernel's arithmetic on the HOST: tests/hostcheck/conv_wide_host.hip compiles the __host__ __device__ bodies of
csrc/snn_conv_wide.hpp (image staging, slab staging, the ordered accumulation, the emit) with hipcc (no GPU needed) and drives them
with the kernel's own schedule: block of 256 output pixels by block, chunk of 8 output channels by chunk, slab of 512 ordered taps
by slab.

  * against oracle.prop_conv2d (the stated order) bit for bit on real-valued weights and bias, over the GPU sweep's shapes, with and
    without accumulate, on the staged and on the unstaged path;
  * whole fixture cases a and c of tests/conv_wide_cases.py (reference-generated) with these bodies in place of the host path's
    F.conv2d: every raster and state array bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import conv_wide_cases as WC
import oracle
from test_conv_wide_host import _bits, _ns, built, check_snapshots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
f32 = np.float32

# (Cin, Cout, KH, KW, stride, pad, H, W, B): the shapes tests/test_gpu_conv_wide.py keeps (its docstring says what each straddles)
SHAPES = [
    (17, 9, 3, 3, 1, 1, 6, 7, 3), (17, 1, 1, 1, 1, 0, 6, 7, 1), (17, 8, 5, 3, 2, 2, 6, 7, 3), (32, 40, 3, 3, 1, 0, 6, 7, 1),
    (64, 40, 3, 3, 1, 1, 6, 7, 3), (64, 130, 1, 1, 2, 2, 6, 7, 1), (100, 9, 5, 3, 1, 1, 6, 7, 3), (100, 8, 3, 3, 2, 2, 6, 7, 1),
    (8, 300, 3, 3, 1, 1, 6, 7, 3), (32, 9, 1, 1, 1, 0, 1, 1, 3), (64, 1, 3, 3, 1, 1, 1, 1, 1), (100, 130, 5, 3, 2, 2, 1, 1, 3),
    (20, 9, 3, 3, 1, 1, 20, 19, 3), (17, 2, 3, 3, 1, 1, 33, 32, 2),
]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libconvwidehost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "conv_wide_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    lib.hostcheck_conv_wide.argtypes = [C.c_void_p] * 4 + [C.c_int] * 11
    lib.hostcheck_conv_wide.restype = C.c_int
    return lib


def conv(host, W, bias, s, stride, pad, prev=None, force_global=False):
    """One compute() of the hostcheck bodies; W [Cout, Cin, KH, KW], s [B, Cin, H, W] u8; returns (out, whether the images were staged)."""
    W, s = np.ascontiguousarray(W, f32), np.ascontiguousarray(s, np.uint8)
    bias = None if bias is None else np.ascontiguousarray(bias, f32)
    B, Cin, H, Wd = s.shape
    Cout, _, KH, KW = W.shape
    OH, OW = (H + 2 * pad - KH) // stride + 1, (Wd + 2 * pad - KW) // stride + 1
    out = np.full((B, Cout, OH, OW), np.nan, f32) if prev is None else np.ascontiguousarray(prev, f32).copy()
    rc = host.hostcheck_conv_wide(W.ctypes.data, None if bias is None else bias.ctypes.data, s.ctypes.data, out.ctypes.data, B, Cin, H, Wd, Cout,
                                  KH, KW, stride, pad, int(prev is not None), int(force_global))
    assert rc in (0, 1), rc
    return out, bool(rc)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bodies_equal_the_stated_order(host, shape):
    Cin, Cout, KH, KW, stride, pad, H, Wd, B = shape
    rng = np.random.default_rng(sum(shape))
    W, bias = rng.standard_normal((Cout, Cin, KH, KW)).astype(f32), rng.standard_normal(Cout).astype(f32)
    staged_seen = set()
    for density in (0.0, 0.01, 0.3, 1.0):
        s = (rng.random((B, Cin, H, Wd)) < density).astype(np.uint8)
        want = oracle.prop_conv2d(W, s, bias=bias, stride=stride, pad=pad)
        for force_global in (False, True):
            got, staged = conv(host, W, bias, s, stride, pad, force_global=force_global)
            staged_seen.add(staged)
            assert np.array_equal(_bits(got), _bits(want)), (shape, density, force_global, int((_bits(got) != _bits(want)).sum()))
        prev = rng.standard_normal(want.shape).astype(f32)
        got, _ = conv(host, W, None, s, stride, pad, prev=prev)
        assert np.array_equal(_bits(got), _bits(prev + oracle.prop_conv2d(W, s, stride=stride, pad=pad))), (shape, density, "accumulate")
    assert False in staged_seen and (True in staged_seen or shape[6] * shape[7] > 1000)


def test_spike_bytes_above_one_are_multiplied(host):
    """The oracle multiplies by the spike byte; so do the bodies (integer weights: every product and sum exact)."""
    rng = np.random.default_rng(3)
    W = rng.integers(-3, 4, size=(9, 20, 3, 3)).astype(f32)
    s = (rng.integers(0, 4, size=(2, 20, 6, 7)) * (rng.random((2, 20, 6, 7)) < 0.3)).astype(np.uint8)
    want = oracle.prop_conv2d(W, s, stride=1, pad=1)
    for force_global in (False, True):
        got, _ = conv(host, W, None, s, 1, 1, force_global=force_global)
        assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", ["a", "c"])
def test_bodies_reproduce_reference_fixture(host, name):
    """The kernel's text over a whole fixture case: what a GPU run of the case computes, without the GPU."""
    g, net = built(name)
    calls = []
    for conn in net.connections.values():
        if type(conn).__name__ == "Conv2dConnection":
            def compute(s, conn=conn):
                x = s.reshape(s.shape[0], *conn.source.shape).to(torch.uint8).numpy()
                out, _ = conv(host, conn.w.detach().numpy(), conn.b.detach().numpy(), x, conn.stride[0], conn.padding[0])
                calls.append(conn.in_channels)
                return torch.from_numpy(out)
            conn._host_compute = compute
    check_snapshots(name, WC.run_case(_ns(), net, name), g)
    assert max(calls) > 16
