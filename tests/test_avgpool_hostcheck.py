"""The average-pooling kernel's arithmetic on the HOST: tests/hostcheck/avgpool_host.hip compiles the __host__ __device__ bodies of
csrc/snn_avgpool.hpp with hipcc (no GPU needed) and drives them output by output, as a thread of the per-output body and as the 64
lanes of the per-wave body do.  Both against F.avg_pool2d, bit for bit, on the geometries of tests/avgpool_cases.py -- output sizes
with ceil_mode, windows clipped to the padded plane, both divisors, divisor_override -- and with accumulate; geometries torch refuses
are refused."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

import avgpool_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libavgpoolhost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "avgpool_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    two = C.POINTER(C.c_int)
    lib.hostcheck_avgpool_size.argtypes = [two] * 4 + [C.c_int, two]
    lib.hostcheck_avgpool_size.restype = C.c_int
    lib.hostcheck_avgpool.argtypes = [C.c_void_p, C.c_void_p, C.c_long] + [two] * 4 + [C.c_int] * 5
    lib.hostcheck_avgpool.restype = C.c_int
    return lib


def _arrays(plane, k, stride, pad):
    pair = lambda v: tuple(v) if isinstance(v, tuple) else (v, v)          # noqa: E731
    return [(C.c_int * 2)(*pair(v)) for v in (plane, k, stride, pad)]


def _pool(host, s, geometry, divisor, body, prev=None):
    plane, k, stride, pad, ceil_mode, include = geometry
    arrays = _arrays(plane, k, stride, pad)
    size = (C.c_int * 2)()
    assert host.hostcheck_avgpool_size(*arrays, int(ceil_mode), size) == 0, geometry
    out = torch.full((s.shape[0], s.shape[1], size[0], size[1]), 7.0) if prev is None else prev.clone().contiguous()
    s = s.to(torch.uint8).contiguous()
    rc = host.hostcheck_avgpool(C.c_void_p(s.data_ptr()), C.c_void_p(out.data_ptr()), s.shape[0] * s.shape[1], *arrays, int(ceil_mode), int(include),
                                0 if divisor is None else divisor, int(prev is not None), body)
    assert rc == 0, (geometry, rc)
    return out


@pytest.mark.parametrize("body", [1, 2], ids=["per-thread", "per-wave"])
def test_both_bodies_equal_torch_on_every_geometry(host, body):
    assert len(AC.GEOMETRIES) * len(AC.DIVISORS) == 576
    for g in AC.GEOMETRIES:
        for divisor in AC.DIVISORS:
            want = AC.reference(g, divisor)
            got = _pool(host, AC.spikes(g[0]), g, divisor, body)
            assert AC.same_bits(got, want), (g, divisor)


def test_accumulate_is_one_rounded_add(host):
    gen = torch.Generator().manual_seed(2)
    for g in AC.GEOMETRIES[::7]:
        want = AC.reference(g)
        prev = torch.rand(want.shape, generator=gen) * 3 - 1
        for body in (1, 2):
            assert AC.same_bits(_pool(host, AC.spikes(g[0]), g, None, body, prev=prev), prev + want), g


def test_whole_plane_window_and_a_negative_divisor(host):
    s = AC.spikes((9, 11))
    for body in (1, 2):
        g = ((9, 11), (9, 11), (9, 11), 0, False, True)
        got = _pool(host, s, g, None, body)
        assert AC.same_bits(got, AC.reference(g)) and AC.same_bits(got, s.float().sum((2, 3), keepdim=True) / 99)
        assert AC.same_bits(_pool(host, s, g, -7, body), AC.reference(g, -7))


def test_what_torch_refuses_is_refused(host):
    size = (C.c_int * 2)()
    ok = lambda plane, k, stride, pad, ceil_mode=0: host.hostcheck_avgpool_size(*_arrays(plane, k, stride, pad), ceil_mode, size)      # noqa: E731
    assert ok((6, 6), (2, 2), (2, 2), 1) == 0 and tuple(size) == (4, 4)
    assert ok((6, 6), (2, 2), (2, 2), 2) == -1                             # torch: pad should be at most half of the kernel size
    assert ok((6, 6), (3, 3), (2, 2), (1, 2)) == -1
    assert ok((2, 6), (3, 3), (1, 1), 0) == -1                             # no window fits: an empty output
    assert ok((6, 6), (0, 2), (1, 1), 0) == -1 and ok((6, 6), (2, 2), (0, 1), 0) == -1 and ok((6, 0), (2, 2), (1, 1), 0) == -1
    assert ok((6, 6), (2, 2), (1, 1), -1) == -1
    assert ok((1 << 15, 1 << 16), (1, 1), (1, 1), 0) == -1                 # a plane beyond 2^30 elements
