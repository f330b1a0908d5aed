"""The bodies of csrc/snn_run_conv_sif.hpp on the HOST: tests/hostcheck/layer_major_host.hip compiles them with hipcc (no GPU needed) and
drives the time loop of snn_run_conv2d_sif_f32 as its per-step scalar restatement -- band words, the stated tap order, the epilogue --
and the body of snn_sif_scan, against the plain float64 reference of layer_major_cases on two of the GPU test's cases."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from layer_major_cases import CASES, khw, reference, shapes, spike_input, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F = C.c_float


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "liblayermajorhost.so")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950",
                    os.path.join(ROOT, "tests", "hostcheck", "layer_major_host.hip"), "-o", out], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    lib.hostcheck_run_conv_sif.argtypes = [C.c_void_p] * 10 + [C.c_int] * 10 + [F, F, F, C.c_int, F, C.c_int, F, F]
    lib.hostcheck_sif_scan.argtypes = [C.c_void_p] * 7 + [C.c_int] * 3 + [F, F, F, C.c_int, F, C.c_int, F, F]
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


# (spec, T, B, refrac, lbound, numerators, density): "c17_16_9x7_refrac" and "stride2 with lbound" of tests/layer_major_cases.py's shapes,
# then its non-square kernels and its paddings beyond half a kernel and of zero, each with the numerators and the input density that
# the table gives it (a refractory period and a lower bound added on two of them)
def _of(name, refrac=0, lbound=None):
    spec, T, B, opt, _ = CASES[name]
    return (spec, T, B, refrac, lbound, opt.get("num", (-4, 12)), opt.get("density", 0.3))


NAMED = ("kh5_kw3", "kh5_kw3_stride2", "kh1_kw3", "kh1_kw3_stride2", "pad_beyond_half", "pad0_cout1")


@pytest.mark.parametrize("spec,T,B,refrac,lbound,num,density", [(((17, 9, 7), [("conv", 16, 3, 1, 1)]), 7, 1, 2, None, (-4, 12), 0.3),
                                                                (((32, 9, 7), [("conv", 20, 3, 2, 1)]), 4, 3, 0, -0.25, (-4, 12), 0.3),
                                                                _of("kh5_kw3"), _of("kh5_kw3_stride2", refrac=2), _of("kh1_kw3"),
                                                                _of("kh1_kw3_stride2", lbound=-0.25), _of("pad_beyond_half"), _of("pad0_cout1")],
                         ids=("spec0-7-1-2-None", "spec1-4-3-0--0.25") + NAMED)
def test_bodies_equal_the_float64_reference(host, request, spec, T, B, refrac, lbound, num, density):
    ws, x = weights(spec, 5, grid=True, num=num), spike_input(spec, T, B, 11, density)
    x[1, 0, 1, 2, 3] = 2                                           # a byte above 1: the stated order takes any byte
    state = {}
    want = reference(spec, ws, x, state, refrac, lbound)[0]
    assert int(want.sum()) > 0
    if request.node.callspec.id in NAMED:                          # (the newer shapes: an equal train must say something)
        assert 0.05 <= float(want.double().mean()) <= 0.95, float(want.double().mean())
    (cout, oh, ow), op = shapes(spec)[0], spec[1][0]
    lif = (1.0, float(refrac), 1.0, int(lbound is not None), float(lbound or 0.0), 0, 0.0, 1.0)
    W, bias, xs = ws[0][0].numpy(), ws[0][1].numpy(), x.numpy()
    n = B * cout * oh * ow

    # the conv + IF time loop
    s0, v, rc, summed, s = np.zeros_like(xs[0]), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    train = np.full((T, n), 9, np.uint8)
    assert host.hostcheck_run_conv_sif(ptr(W), ptr(bias), ptr(s0), ptr(xs), ptr(train), ptr(v), ptr(rc), ptr(summed), None, ptr(s), T, B,
                                       *spec[0], cout, *khw(op[2]), op[3], op[4], *lif) == 0
    assert np.array_equal(train.reshape(want.shape), want.numpy()) and np.array_equal(s, train[-1])
    assert np.array_equal(v.astype(np.float64), state["v"][0].numpy().ravel()) and np.array_equal(rc.astype(np.float64), state["rc"][0].numpy().ravel())
    assert np.array_equal(summed.astype(np.float64), state["summed"].numpy().ravel())

    # the scan over currents an operator left (here: the exact float64 convolution, which float32 holds)
    prev = torch.cat((torch.zeros_like(x[:1]), x[:-1])).double().reshape(T * B, *spec[0])
    I = torch.nn.functional.conv2d(prev, ws[0][0].double(), ws[0][1].double(), stride=op[3], padding=op[4]).float().numpy().reshape(T, n)
    v2, rc2, sum2, s2, train2 = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8), np.full((T, n), 9, np.uint8)
    assert host.hostcheck_sif_scan(ptr(v2), ptr(rc2), ptr(s2), None, ptr(sum2), ptr(np.ascontiguousarray(I)), ptr(train2), T, B, n // B, *lif) == 0
    assert np.array_equal(train2, train) and np.array_equal(v2, v) and np.array_equal(rc2, rc) and np.array_equal(sum2, summed) and np.array_equal(s2, s)
