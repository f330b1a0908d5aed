"""The pooling and mean-field kernels' arithmetic on the HOST: tests/hostcheck/pool_host.hip compiles the __host__ __device__ bodies
of csrc/snn_pool.hpp (rate update, window scan and index rule, gather, mean and product) with hipcc (no GPU needed) and drives them
plane by plane, as the kernels do.

  * the index rule against F.max_pool1d / 2d / 3d(..., return_indices=True) on random geometries (kernel, stride, padding, dilation
    drawn per axis) and four kinds of data: small integers (ties in most windows), those with NaN sprinkled in, with -inf, and
    all -inf;
  * whole compute() sequences (rate update + pooling + gather, with and without accumulate) against torch;
  * whole fixture cases a, b, e and h of tests/pool_cases.py (reference-generated) with these bodies in place of the host path's
    torch expressions: raster, every state tensor, firing_rates, bit for bit;
  * the mean-field bodies against torch's own mean at sizes around 2^24 and counts 0 .. numel."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_cases as PC
from test_pool_host import _bits, _ns, check_snapshots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libpoolhost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "pool_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp, three = C.c_void_p, C.POINTER(C.c_int)
    lib.hostcheck_pool.argtypes = [vp, vp, vp, C.c_long] + [three] * 5 + [C.c_float, C.c_int]
    lib.hostcheck_pool_indices.argtypes = [vp, vp, C.c_long] + [three] * 5
    lib.hostcheck_meanfield.argtypes = [vp, C.c_int, vp, vp, C.c_long, C.c_long, C.c_int]
    for fn in (lib.hostcheck_pool, lib.hostcheck_pool_indices, lib.hostcheck_meanfield):
        fn.restype = C.c_int
    return lib


def _p(t):
    return C.c_void_p(t.data_ptr())


def _pool(host, fr, s, k, stride, pad, dil, decay, prev=None):
    """One compute() of the hostcheck bodies: fr [B, C, *spatial] updated in place; returns out [B, C, *pooled]."""
    from bindsnet_amd import ops
    arrays, pooled = ops.pool_geometry(fr.shape[2:], k, stride, pad, dil)
    out = torch.zeros(*fr.shape[:2], *pooled) if prev is None else prev.clone().contiguous()
    s = s.to(torch.uint8).reshape(fr.shape).contiguous()
    assert host.hostcheck_pool(_p(fr), _p(s), _p(out), fr.shape[0] * fr.shape[1], *arrays, float(decay), int(prev is not None)) == 0
    return out


def _geometry(rng, nd):
    """A random geometry torch accepts: per axis a kernel, stride, dilation, a padding of at most half the kernel and a size that
    leaves at least one pooled position."""
    k = [int(rng.integers(1, 5)) for _ in range(nd)]
    d = [int(rng.integers(1, 4)) for _ in range(nd)]
    s = [int(rng.integers(1, 4)) for _ in range(nd)]
    p = [int(rng.integers(0, k[a] // 2 + 1)) for a in range(nd)]
    size = [max(1, d[a] * (k[a] - 1) + 1 - 2 * p[a]) + int(rng.integers(0, 7)) for a in range(nd)]
    if (PC.window_taps(dict(nd=nd, shape=(1, *size), k=k, s=s, p=p, d=d))[:, 0] < 0).any():
        return _geometry(rng, nd)          # a dilated window that misses the plane: torch's index is outside the plane, the classes refuse it
    return size, k, s, p, d


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_index_rule_equals_torch(host, nd):
    from bindsnet_amd import ops
    rng = np.random.default_rng(40 + nd)
    pool = getattr(F, f"max_pool{nd}d")
    seen_nonfirst = seen_nan = 0
    for trial in range(60):
        size, k, s, p, d = _geometry(rng, nd)
        base = torch.from_numpy(rng.integers(0, 3, size=(2, 3, *size)).astype(np.float32))
        for kind in ("ties", "nan", "neg_inf", "all_neg_inf"):
            fr = base.clone()
            if kind == "nan":
                fr[torch.from_numpy(rng.random(fr.shape) < 0.2)] = float("nan")
            elif kind == "neg_inf":
                fr[torch.from_numpy(rng.random(fr.shape) < 0.5)] = float("-inf")
            elif kind == "all_neg_inf":
                fr.fill_(float("-inf"))
            _, want = pool(fr, kernel_size=k, stride=s, padding=p, dilation=d, return_indices=True)
            arrays, pooled = ops.pool_geometry(size, k, s, p, d)
            assert tuple(want.shape[2:]) == pooled
            got = torch.zeros(want.shape, dtype=torch.int64)
            assert host.hostcheck_pool_indices(_p(fr), _p(got), 6, *arrays) == 0
            assert torch.equal(got, want), f"{nd}-d, size {size} k {k} s {s} p {p} d {d}, {kind}: {(got != want).sum()} indices differ"
            if kind == "ties":
                first = pool(torch.zeros_like(fr), kernel_size=k, stride=s, padding=p, dilation=d, return_indices=True)[1]
                seen_nonfirst += int((want != first).sum())
            seen_nan += int(torch.isnan(fr.flatten(2).gather(2, want.flatten(2))).sum()) if kind == "nan" else 0
    assert seen_nonfirst > 100 and seen_nan > 100


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_compute_sequences_equal_torch(host, nd):
    rng = np.random.default_rng(70 + nd)
    pool = getattr(F, f"max_pool{nd}d")
    for trial in range(12):
        size, k, s, p, d = _geometry(rng, nd)
        decay = float(rng.choice([0.0, 0.1, 0.37, 1.0]))
        fr_t = torch.zeros(2, 3, *size)
        fr_h = fr_t.clone()
        for step in range(6):
            spikes = torch.from_numpy((rng.random(fr_t.shape) < 0.4).astype(np.uint8))
            fr_t -= decay * fr_t
            fr_t += spikes.float()
            _, idx = pool(fr_t, kernel_size=k, stride=s, padding=p, dilation=d, return_indices=True)
            want = spikes.flatten(2).gather(2, idx.flatten(2)).view_as(idx).float()
            prev = torch.from_numpy(rng.random(want.shape).astype(np.float32)) if step % 2 else None
            got = _pool(host, fr_h, spikes, k, s, p, d, decay, prev=prev)
            assert np.array_equal(_bits(fr_h.numpy()), _bits(fr_t.numpy())), "firing rates"
            assert np.array_equal(_bits(got.numpy()), _bits((want if prev is None else prev + want).numpy())), "pooled spikes"


@pytest.mark.parametrize("name", ["a", "b", "e", "h"])
def test_bodies_reproduce_reference_fixture(host, name):
    """The kernels' text over a whole fixture case: what a GPU run of the case computes, without the GPU."""
    from bindsnet_amd.network.monitors import Monitor
    net = PC.build(_ns(), name)
    for conn in net.connections.values():
        if hasattr(conn, "firing_rates"):
            def compute(s, conn=conn):
                fr = conn._rates(s.shape[0], s.device)
                return _pool(host, fr, s, *conn._fields(), float(conn.decay))
            conn._host_compute = compute
        elif type(conn).__name__ == "MeanFieldConnection":
            def compute(s, conn=conn):
                B = s.shape[0]
                out = torch.zeros(B, conn.target.n)
                sb = s.to(torch.uint8).contiguous()
                assert host.hostcheck_meanfield(_p(conn.w.data), conn.w.numel(), _p(sb), _p(out), sb.numel(), out.numel(), 0) == 0
                return out.view(B, *conn.target.shape)
            conn._host_compute = compute
    check_snapshots(name, PC.run_case(net, name, Monitor))


def test_meanfield_bodies_equal_torch_mean(host):
    rng = np.random.default_rng(9)
    threads = torch.get_num_threads()
    try:
        for numel, n_threads in ((1, 1), (7, 1), (1000, 1), ((1 << 24) - 3, 1), (1 << 24, 1), (1 << 24, max(2, min(8, threads)))):
            torch.set_num_threads(n_threads)
            for density in (0.0, 0.3, 1.0):
                s = torch.from_numpy((rng.random(numel) < density).astype(np.uint8)) if 0.0 < density < 1.0 else \
                    torch.full((numel,), int(density), dtype=torch.uint8)
                w = torch.tensor([-0.5, 3.0, 0.1])
                prev = torch.tensor([1.0, -2.0, 0.25])
                mean = s.float().mean()
                for mode, want in ((2, mean * w), (0, torch.zeros(3) + mean * w), (1, prev + mean * w)):
                    out = prev.clone()
                    assert host.hostcheck_meanfield(_p(w), 3, _p(s), _p(out), numel, 3, mode) == 0
                    assert np.array_equal(_bits(out.numpy()), _bits(want.numpy())), (numel, density, mode)
    finally:
        torch.set_num_threads(threads)
