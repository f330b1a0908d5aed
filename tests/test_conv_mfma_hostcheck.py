"""The bodies of csrc/snn_conv_mfma.hpp on the HOST: tests/hostcheck/conv_mfma_host.hip compiles them with hipcc (no GPU needed) and
drives them with the kernel's schedule -- band staging and census, tap map, slab slots and weights, the fmaf chain in the padded K
order with its slab cuts, the scalar body -- against the numpy restatement of the stated order, bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conv_mfma_cases import SHAPES, case, khw, stated_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libconvmfmahost.so")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950",
                    os.path.join(ROOT, "tests", "hostcheck", "conv_mfma_host.hip"), "-o", out], check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    lib.hostcheck_conv_mfma.argtypes = [C.c_void_p] * 4 + [C.c_int] * 11 + [C.c_void_p]
    return lib


@pytest.mark.parametrize("shape,NT", [(SHAPES[0], 1), (SHAPES[1], 2), (SHAPES[8], 1), (SHAPES[9], 2), (SHAPES[10], 1), (SHAPES[11], 1)])
@pytest.mark.parametrize("levels", (2, 4), ids=("chain", "scalar"))
def test_bodies_equal_the_stated_order(host, shape, NT, levels):
    Cin, Cout, K, stride, pad, H, Wd, B = shape
    W, bias, s, oshape = case(shape, seed=levels, levels=levels, density=0.4)
    out, cnt = np.full(oshape, 7.5, np.float32), np.zeros(2, np.int32)
    assert host.hostcheck_conv_mfma(W.ctypes.data, bias.ctypes.data, s.ctypes.data, out.ctypes.data, B, Cin, H, Wd, Cout, *khw(K), stride, pad,
                                    0, NT, cnt.ctypes.data) == 0
    assert np.array_equal(out.view(np.uint32), stated_order(W, s, bias, stride, pad).view(np.uint32))
    assert (cnt[0] > 0 and cnt[1] == 0) if levels == 2 else (cnt[0] == 0 and cnt[1] > 0)
