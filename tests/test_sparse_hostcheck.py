"""SparseConnection's propagation kernel on the HOST: tests/hostcheck/sparse_host.hip compiles the __host__ __device__ bodies of
csrc/snn_sparse.hpp (segment look-up, ordered walk, accumulate, finish) with hipcc (no GPU needed) and drives them one (column tile,
sample) pair at a time, as k_prop_sparse's waves do.

  * whole fixture cases a, c, e and g of tests/sparse_cases.py (reference-generated) with the walk in place of the host path's
    product: raster, every final state tensor, bit for bit;
  * the walk against torch's own `s.float() @ w_sparse` on random matrices: EVERY N from 1 to 130 at source counts around 64, 256
    and 1024, and target counts around the 256-column tile."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import sparse_cases as SC
from test_sparse_host import _bits, _ns, check_snapshots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libsparsehost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "sparse_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.hostcheck_sparse_prop.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp] + [C.c_int] * 5
    lib.hostcheck_sparse_prop.restype = C.c_int
    return lib


def _walk(host, compiled, s, N, bias=None, prev=None, lanes=64):
    """out [B, N] of the hostcheck walk for spikes s [B, Nin] (uint8 tensor); prev: what `out` holds with accumulate.  lanes == 1: one
    worker walks the whole segment list; lanes == 64: segment by segment, the kernel's entry <-> lane mapping."""
    ptr, col, val = (t.contiguous() for t in compiled)
    s = s.reshape(s.shape[0], -1).to(torch.uint8).contiguous()
    B, Nin = s.shape
    out = torch.zeros(B, N) if prev is None else prev.clone().contiguous()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
    rc = host.hostcheck_sparse_prop(p(ptr), p(col) if val.numel() else None, p(val) if val.numel() else None, val.numel(),
                                    p(None if bias is None else bias.contiguous()), p(s), p(out), B, Nin, N, int(prev is not None), lanes)
    assert rc == 0
    return out


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("name", ["a", "c", "e", "g"])
def test_walk_reproduces_reference_fixture(host, name, lanes):
    """The kernel's per-lane text over a whole fixture case: what a GPU run of the case computes, without the GPU."""
    from bindsnet_amd import ops
    from bindsnet_amd.network.monitors import Monitor
    net = SC.build(_ns(), name)
    for conn in net.connections.values():
        compiled = ops.sparse_compile(conn.w)

        def compute(s, conn=conn, compiled=compiled):
            return _walk(host, compiled, s, conn.target.n, bias=None if conn.b is None else conn.b.data, lanes=lanes).view(s.shape[0], *conn.target.shape)
        conn._host_compute = compute
    check_snapshots(name, SC.run_case(net, name, Monitor))


def _against_torch(host, Nin, N, seed, lanes=64):
    from bindsnet_amd import ops
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(Nin, N, generator=g) - 0.4) * (torch.rand(Nin, N, generator=g) < 0.2)
    ws = w.to_sparse()
    s = (torch.rand(3, Nin, generator=g) < 0.3).to(torch.uint8)
    bias = torch.rand(N, generator=g) - 0.5 if seed % 2 else None
    prev = torch.rand(3, N, generator=g) if seed % 3 == 0 else None
    want = s.float() @ ws
    if bias is not None:
        want = want + bias
    if prev is not None:
        want = prev + want
    got = _walk(host, ops.sparse_compile(ws), s, N, bias=bias, prev=prev, lanes=lanes)
    bad = np.flatnonzero(_bits(got.numpy()).reshape(-1) != _bits(want.numpy()).reshape(-1))
    assert bad.size == 0, f"Nin = {Nin}, N = {N}: {bad.size} of {3 * N} sums differ from torch (first {bad[:5]})"


@pytest.mark.parametrize("Nin", [63, 64, 65, 255, 257, 1023, 1024, 1025])
def test_walk_equals_torch_sparse_product_for_every_n(host, Nin):
    for N in range(1, 131):
        _against_torch(host, Nin, N, 1000 * Nin + N, lanes=1 if N % 2 else 64)


@pytest.mark.parametrize("N", [255, 256, 257, 513, 700])
def test_walk_equals_torch_across_column_tiles(host, N):
    for Nin, lanes in ((70, 64), (1100, 64), (2100, 1)):
        _against_torch(host, Nin, N, 7 * N + Nin, lanes=lanes)


def test_walk_at_one_and_many_threads(host):
    n = torch.get_num_threads()
    try:
        for threads in (1, max(2, min(8, n))):
            torch.set_num_threads(threads)
            _against_torch(host, 1500, 300, 4242)
    finally:
        torch.set_num_threads(n)


def test_header_tile_matches_the_binding():
    from bindsnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snnhip.h")).read()
    assert f"#define SNN_SPARSE_TJ {_lib.SPARSE_TJ}\n" in hdr
    hpp = open(os.path.join(ROOT, "bindsnet_amd", "csrc", "snn_sparse.hpp")).read()
    assert f"constexpr int kSparseTJ = {_lib.SPARSE_TJ};" in hpp
