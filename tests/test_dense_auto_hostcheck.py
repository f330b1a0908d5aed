"""What snn_prop_dense_auto_f32 decides with, on the HOST: tests/hostcheck/dense_auto_host.hip compiles the __host__ __device__ text of
csrc/snn_dense_auto.hpp with hipcc (no GPU needed).

  * the census of every tile of 16 samples equals numpy's count of non-zero bytes (the largest of the tile's valid rows) and numpy's
    "any byte above 1", over the operator sweep's shapes: tail rows, Nin not a multiple of 16, rows that are not 16-byte aligned;
  * the cost rule is monotone in the event count, never says matrix for a tile with a byte above 1 and says event for a silent tile,
    in every mode;
  * the fused multiply-add chain (the MFMA) equals the multiply-then-add chain (the event-driven kernel) bit for bit for 0/1 factors
    over signed, subnormal and zero weights -- the stated reason the two bodies agree -- and does not for a factor of 3."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BS = (1, 15, 16, 17, 33)
NINS = (1, 15, 16, 17, 100, 1024, 1025, 1041)
DENSITIES = (0.0, 0.02, 0.3, 1.0)
MODES = (0, 1, 2)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libdenseautohost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "dense_auto_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    lib.hostcheck_census.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.hostcheck_census.restype = C.c_int
    lib.hostcheck_use_matrix.argtypes = [C.c_int] * 7
    lib.hostcheck_use_matrix.restype = C.c_int
    lib.hostcheck_chains.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.hostcheck_chains.restype = None
    return lib


def numpy_census(s):
    B = s.shape[0]
    tiles = [s[m0:m0 + 16] for m0 in range(0, B, 16)]
    return np.array([[int((t != 0).sum(axis=1).max()), int((t > 1).any())] for t in tiles], np.int32)


@pytest.mark.parametrize("Nin", NINS)
def test_census_equals_numpy(host, Nin):
    rs = np.random.RandomState(7 * Nin)
    for B in BS:
        for dens in DENSITIES:
            for twos in (0, 1, 5):                  # bytes above 1 sprinkled in, the very last byte of the last row among them
                for shift in (0, 3):                # the array starts 16-byte aligned / 3 bytes behind that
                    s = (rs.uniform(size=(B, Nin)) < dens).astype(np.uint8)
                    for k in range(twos):
                        s[rs.randint(B), rs.randint(Nin)] = rs.randint(2, 256)
                    if twos == 1:
                        s[B - 1, Nin - 1] = 2
                    buf = np.zeros(B * Nin + 64, np.uint8)
                    off = (-buf.ctypes.data) % 16 + shift
                    buf[off:off + B * Nin] = s.ravel()
                    got = np.full(((B + 15) // 16, 2), -1, np.int32)
                    assert host.hostcheck_census(C.c_void_p(buf.ctypes.data + off), B, Nin, C.c_void_p(got.ctypes.data)) == 0
                    np.testing.assert_array_equal(got, numpy_census(s), err_msg=f"B={B} Nin={Nin} dens={dens} twos={twos} shift={shift}")


SHAPES = [(16, 1600, 256), (1, 784, 256), (16, 784, 256), (16, 256, 128), (1, 6400, 100), (16, 6400, 100), (128, 784, 1600),
          (16, 6400, 500), (1024, 784, 1600), (17, 64, 48), (33, 1041, 130), (1, 1, 1)]


@pytest.mark.parametrize("B,Nin,N", SHAPES)
def test_rule_properties(host, B, Nin, N):
    for rows in sorted({1, min(16, B), (B - 1) % 16 + 1}):
        for mode in MODES:
            said = [host.hostcheck_use_matrix(c, 0, rows, Nin, N, B, mode) for c in range(Nin + 1)]
            assert set(said) <= {0, 1}
            assert said == sorted(said), f"not monotone in the event count: mode {mode}"
            assert said[0] == 0, "a silent tile takes the event body"
            assert all(host.hostcheck_use_matrix(c, 1, rows, Nin, N, B, mode) == 0 for c in range(Nin + 1)), "matrix with a byte above 1"
            if mode == 1:
                assert not any(said)
            if mode == 2:
                assert all(said[1:])
        assert host.hostcheck_use_matrix(Nin, 0, 0, Nin, N, B, 0) == 0      # no valid row


def test_rule_ends_at_the_acceptance_shape(host):
    """B = 16, 1600 -> 256 (tests/test_gpu_dense_auto.py asserts the same on the device): at 50 % the walk is 800 rows against 100
    rounds, at 1 % 16 against 100.  Every count a Bernoulli row of that density can plausibly have is on the same side."""
    for c in range(640, 961):
        assert host.hostcheck_use_matrix(c, 0, 16, 1600, 256, 16, 0) == 1
    for c in range(0, 41):
        assert host.hostcheck_use_matrix(c, 0, 16, 1600, 256, 16, 0) == 0


def _weights(rs, n):
    w = rs.uniform(-1.0, 1.0, n).astype(np.float32)
    kinds = rs.randint(0, 8, n)
    w[kinds == 0] = 0.0
    w[kinds == 1] = -0.0
    sub = (rs.randint(1, 1 << 23, n).astype(np.uint32) | (rs.randint(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    w[kinds == 2] = sub[kinds == 2]                             # subnormals of either sign
    w[kinds == 3] *= np.float32(1e-30)
    w[kinds == 4] *= np.float32(3e4)
    return w


def test_fma_chain_equals_mul_add_chain_for_01_factors(host):
    rs = np.random.RandomState(11)
    a, b = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    for n in (1, 2, 3, 15, 16, 17, 100, 1041):
        for dens in (0.0, 0.02, 0.3, 1.0):
            for rep in range(8):
                w = _weights(rs, n)
                s = (rs.uniform(size=n) < dens).astype(np.uint8)
                host.hostcheck_chains(C.c_void_p(s.ctypes.data), C.c_void_p(w.ctypes.data), n, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data))
                assert a[0] == b[0], (n, dens, rep, hex(a[0]), hex(b[0]))
                # numpy's own sequential sum of the selected weights: the ordered sum the oracle states
                acc = np.float32(0.0)
                for k in np.flatnonzero(s):
                    acc = np.float32(acc + w[k])
                assert a[0] == np.array([acc], np.float32).view(np.uint32)[0]
    # another factor separates them: 3 * w is rounded before the add in one chain and not in the other
    n = 1041
    diff3 = 0
    for rep in range(8):
        w3 = rs.uniform(0.3, 1.0, n).astype(np.float32)
        s3 = np.full(n, 3, np.uint8)
        host.hostcheck_chains(C.c_void_p(s3.ctypes.data), C.c_void_p(w3.ctypes.data), n, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data))
        diff3 += int(a[0] != b[0])
    assert diff3 > 0, "a factor of 3 rounds twice in one chain and once in the other"
