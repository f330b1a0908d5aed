"""The real-valued Input's kernel arithmetic on the HOST: tests/hostcheck/real_host.hip compiles the __host__ __device__ bodies the
kernels of csrc/snn_real.hip run (csrc/snn_real.hpp) with hipcc (no GPU, no sanitizer) and drives them element by element, as the
kernels' threads do -- the dense chains in sample tiles with the per-tile zero skip, the convolution's chains from the filters'
staged layout and from the plain one, the Input's trace.  Compared bit for bit with the numpy stated order of tests/analog_cases.py
over the operator sweep the device test uses, and with the `tr_*` fixtures the reference produced."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import analog_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "librealhost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "real_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    lib.hostcheck_dense_real.argtypes = [vp] * 4 + [i] * 5
    lib.hostcheck_conv2d_real.argtypes = [vp] * 4 + [i] * 11
    lib.hostcheck_input_real.argtypes = [vp, vp, i, i, i, f, f, i, vp, vp, vp]
    lib.hostcheck_dense_real.restype = lib.hostcheck_conv2d_real.restype = C.c_int
    lib.hostcheck_input_real.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("nin", AC.DENSE_NIN)
def test_dense_bodies_equal_the_stated_order(host, nin):
    for c in AC.dense_sweep(nin):
        B, n = c["x"].shape[0], c["w"].shape[1]
        for tile in (2, 0):
            out = c["prev"].copy() if c["prev"] is not None else np.full((B, n), np.nan, np.float32)
            assert host.hostcheck_dense_real(_p(c["w"]), _p(c["b"]), _p(c["x"]), _p(out), B, nin, n, int(c["prev"] is not None), tile) == 0
            assert _same(out, c["want"]), (nin, n, B, c["b"] is not None, c["prev"] is not None, tile)


@pytest.mark.parametrize("img", AC.CONV_IMG)
@pytest.mark.parametrize("cin", AC.CONV_CIN)
def test_conv2d_bodies_equal_the_stated_order(host, cin, img):
    for c in AC.conv_sweep(cin, img):
        B, cout, K = c["x"].shape[0], c["w"].shape[0], c["w"].shape[2]
        for staged in (1, 0):
            out = c["prev"].copy() if c["prev"] is not None else np.full(c["want"].shape, np.nan, np.float32)
            assert host.hostcheck_conv2d_real(_p(c["w"]), _p(c["b"]), _p(c["x"]), _p(out), B, cin, img[0], img[1], cout, K, K, c["stride"], c["pad"],
                                              int(c["prev"] is not None), staged) == 0
            assert _same(out, c["want"]), (cin, img, K, c["stride"], c["pad"], cout, B, staged)


def test_input_trace_body_equals_the_stated_order(host):
    for c in AC.step_sweep():
        T, B, n = c["s"].shape
        x, rec = c["x0"].copy(), np.empty((T, B, n), np.float32)
        vec = c["scale"] if c["mode"] == "pv" else None
        host.hostcheck_input_real(_p(c["s"]), _p(x), T, B, n, c["decay"], 0.0 if vec is not None else float(c["scale"]), int(c["additive"]), None, _p(vec), _p(rec))
        assert _same(rec, c["want"]) and _same(x, c["want"][-1]), (n, B, c["mode"])


@pytest.mark.parametrize("name", list(AC.TRACE))
def test_input_trace_body_equals_the_reference(host, name):
    """The `tr_*` fixtures: the reference's per-step trace of an Input fed real values."""
    g = AC.gold(name)
    inp, shape, T, B, _ = AC.case_meta(name)
    decay = float(torch.exp(-torch.tensor(1.0) / torch.tensor(AC.LIF["tc_trace"])))
    scale = AC.trace_scale(name)
    vec = scale.numpy().astype(np.float32) if isinstance(scale, torch.Tensor) else None
    for r in range(AC.N_IN):
        s = AC.case_runs(name, r)[0]
        x, rec = np.zeros((B, shape[0]), np.float32), np.empty((T, B, shape[0]), np.float32)
        host.hostcheck_input_real(_p(s), _p(x), T, B, shape[0], decay, 0.0 if vec is not None else float(scale), int(AC.TRACE[name]["mode"] != "set"),
                                  None, _p(vec), _p(rec))
        assert _same(rec, g[f"r{r}_X_xrec"].reshape(rec.shape)) and _same(x, g[f"r{r}_X_x"].reshape(x.shape))
