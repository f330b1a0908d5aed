"""The bodies of csrc/snn_run_dense_sif.hpp on the HOST: tests/hostcheck/run_dense_sif_host.hip compiles them with hipcc (no GPU needed)
and drives the kernel's split -- staging and masking, the row-to-lane map, the scan's hand-off from lane group to lane group and the
scalar body -- against the plain float64 reference of tests/run_dense_sif_cases.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from run_dense_sif_cases import SHAPES, TRACES, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F = C.c_float


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "librundensehost.so")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950",
                    os.path.join(ROOT, "tests", "hostcheck", "run_dense_sif_host.hip"), "-o", out], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    lib.hostcheck_run_dense_sif.argtypes = [C.c_void_p] * 10 + [C.c_int] * 4 + [F, F, C.c_int, F, F, C.POINTER(C.c_int)]
    return lib


@pytest.mark.parametrize("bias,refrac,traces,two", [(True, 0, False, False), (False, 2, True, True)], ids=("plain", "bare_byte2"))
@pytest.mark.parametrize("name", list(SHAPES))
def test_bodies_equal_the_float64_reference(host, name, bias, refrac, traces, two):
    T, B, Nin, N = SHAPES[name]
    W, b, s0, x, ent, want, state = case(name, bias, refrac, traces, two)
    f32 = lambda k: np.ascontiguousarray(ent[k].numpy().astype(np.float32))      # noqa: E731
    v, rc, summed, tr = f32("v"), f32("rc"), f32("summed"), f32("x")
    s, train, xs = np.full((B, N), 9, np.uint8), np.full((2 * T, B, N), 9, np.uint8), x.numpy()
    ptr = lambda a: None if a is None else a.ctypes.data                        # noqa: E731
    scalar = [C.c_int(-1), C.c_int(-1)]
    for run, start in enumerate((s0.numpy(), xs[T - 1])):                        # two calls of T on the same state
        frames = np.ascontiguousarray(xs[run * T:(run + 1) * T - 1]) if T > 1 else None
        assert host.hostcheck_run_dense_sif(ptr(W.numpy()), ptr(None if b is None else b.numpy()), ptr(np.ascontiguousarray(start)), ptr(frames),
                                            ptr(train[run * T:]), ptr(v), ptr(rc), ptr(summed), ptr(tr) if traces else None, ptr(s), T, B, Nin, N,
                                            1.0, float(refrac), int(traces), TRACES[0], TRACES[1], C.byref(scalar[run])) == 0
    assert scalar[0].value == 0 and scalar[1].value == (int(two) * -(-N // 64))   # the byte 2 feeds one super block of the second call
    if T * B * N >= 64:
        assert 0.02 < want.double().mean() < 0.98
    assert np.array_equal(train, want.numpy()) and np.array_equal(s, train[-1])
    for got, key in ((v, "v"), (rc, "rc"), (summed, "summed")) + (((tr, "x"),) if traces else ()):
        ref = state[key] if key == "summed" else state[key][0]
        assert np.array_equal(got.astype(np.float64), ref.numpy()), key
