"""The CSRM kernels' arithmetic on the HOST: tests/hostcheck/csrm_host.hip compiles the __host__ __device__ bodies of
csrc/snn_csrm.hpp (ring slot rule, ascending gather, store / accumulate, the layer's step) with hipcc (no GPU needed) and drives
them as the kernels do.

  * whole fixture cases of tests/csrm_cases.py with these bodies in place of the host path's torch expressions (the ring and its
    head included: `conn.s_w` is read back through them) against the stated order (csrm_cases.stated_run): raster, v, theta,
    last_spikes, s_w, traces and w, bit for bit;
  * the accumulate flag, a window of one slot, a source count that is no multiple of the 256-entry list, more than 256 columns."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import csrm_cases as CC
from test_csrm_host import build, check_snapshots, decays, gold, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libcsrmhost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "csrm_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp, i = C.c_void_p, C.c_int
    lib.hostcheck_prop_window.argtypes = [vp, vp, vp, i, vp, vp, i, i, i, i, i]
    lib.hostcheck_csrm_step.argtypes = [vp] * 7 + [i, vp, i, i, i, vp, vp, vp]
    lib.hostcheck_prop_window.restype = lib.hostcheck_csrm_step.restype = i
    return lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def prop_window(host, W, bias, ring, head, s, out=None):
    """One snn_prop_window_f32 on the host bodies; returns out [B, Wres, N] (accumulated into `out` when given)."""
    B, Wn, Nin = ring.shape
    acc = out is not None
    out = out if acc else torch.full((B, Wn, W.shape[1]), float("nan"))
    s = s.reshape(B, Nin).to(torch.uint8).contiguous()
    assert host.hostcheck_prop_window(_p(W), _p(bias), _p(ring), head, _p(s), _p(out), B, Wn, Nin, W.shape[1], int(acc)) == 0
    return out


def patched(host, monkeypatch):
    """The package's host path with the two torch restatements replaced by the kernel bodies."""
    from bindsnet_amd.network import host_path

    def window(conn, s):
        B, wres = s.shape[0], int(conn.target.res_window_size)
        win = conn.__dict__.get("_win")
        if win is None or win["ring"] is None:
            win = conn.__dict__["_win"] = {"host": None, "ring": torch.zeros(B, wres, conn.source.n, dtype=torch.uint8), "head": 0}
        out = prop_window(host, conn.w.data, None if conn.b is None else conn.b.data, win["ring"], win["head"], s)
        win["head"] = (win["head"] + 1) % wres
        return out.view(B, wres, *conn.target.shape)

    def step(layer, x):
        pv = {}
        from bindsnet_amd import _lib
        p = layer._csrm_params(pv)
        vecs = _lib.pervec(pv)
        B = layer.v.shape[0]
        s = torch.zeros(B, layer.n, dtype=torch.uint8)
        x = x.reshape(B, -1, layer.n).contiguous()
        assert host.hostcheck_csrm_step(_p(layer.v), _p(s), _p(layer.x), _p(layer.theta), _p(x), _p(layer.last_spikes), _p(layer.resKernel),
                                        layer.resKernel.numel(), _p(layer.refKernel), layer.refKernel.numel(), B, layer.n, C.byref(p),
                                        None if vecs is None else C.byref(vecs), None) == 0
        layer.s = s.bool().view(B, *layer.shape)

    monkeypatch.setattr(host_path, "_propagate_window", window)
    monkeypatch.setattr(host_path, "_step_csrm", step)


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_kernel_bodies_equal_the_stated_order_on_fixture_cases(host, monkeypatch, name):
    from bindsnet_amd.network.monitors import Monitor
    patched(host, monkeypatch)
    c, seed = CC.CASES[name], int(gold(name)["seed"])
    snaps = CC.run_case(build(name), c, seed, Monitor)
    check_snapshots(name, snaps, against=CC.stated_run(c, seed, decays=decays(name)), v_exact=True)


@pytest.mark.parametrize("B,Wn,Nin,N", [(1, 1, 5, 3), (2, 4, 300, 7), (3, 33, 50, 257), (1, 20, 784, 300)])
def test_window_propagation_and_accumulate(host, B, Wn, Nin, N):
    rng = np.random.default_rng(B * 1000 + Wn)
    W = torch.from_numpy(rng.standard_normal((Nin, N)).astype(np.float32))
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
    ring = torch.zeros(B, Wn, Nin, dtype=torch.uint8)
    window = torch.zeros(B, Wn, Nin)
    head = 0
    for t in range(Wn + 3):
        s = torch.from_numpy((rng.random((B, Nin)) < (0.0 if t == 1 else 1.0 if t == 2 else 0.2)).astype(np.uint8))
        window = torch.cat((window[:, 1:], s[:, None].float()), 1)
        before = torch.from_numpy(rng.standard_normal((B, Wn, N)).astype(np.float32))
        got = prop_window(host, W, bias, ring.clone(), head, s)
        got_acc = prop_window(host, W, None, ring, head, s, out=before.clone())
        head = (head + 1) % Wn
        same(got.numpy(), CC.window_currents(None, window, W, bias).numpy(), f"step {t}: window currents")
        same(got_acc.numpy(), CC.window_currents(before, window, W).numpy(), f"step {t}: accumulated window currents")
        same(torch.cat((ring[:, head:], ring[:, :head]), 1).float().numpy(), window.numpy(), f"step {t}: the ring read oldest slot first")
