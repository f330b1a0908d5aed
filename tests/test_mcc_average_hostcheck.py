"""The averaged MCC rule kernels' arithmetic on the HOST: tests/hostcheck/average_host.hip compiles the __host__ __device__ bodies of
csrc/snn_average.hpp with hipcc (no GPU needed) and drives them element by element, as the kernels' threads do.

  * the ring's mean against torch.mean(buf, 0) for K in {1, 2, 31, 32, 33, 255, 256} and E in {1, 5, 31, 32, 33, 1073}: every column
    class of ATen's sum(dim=0) (the inner reduction at E = 1, the 4..7 class, cascade and row_sum columns), one division by K;
  * the fixture cases of tests/mcc_average_cases.py (reference-generated) with these bodies in place of the host path's torch
    statements: rasters, W, rings, indices, p_plus, p_minus, eligibility_trace, bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mcc_average_cases as AC
from test_mcc_average_host import ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libaveragehost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "average_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    lib.hostcheck_avg_mean.argtypes = [vp, i, C.c_long, vp]
    lib.hostcheck_avg_postpre.argtypes = [vp] * 5 + [i, i, i, f, f, f, f, i, f, i, f, i, vp, vp, i, i, i, i]
    lib.hostcheck_avg_mstdp.argtypes = [vp] * 7 + [i, i, i, f, vp, f, f, f, f, f, f, i, f, i, f, i, vp, i, i, i]
    lib.hostcheck_avg_mstdpet.argtypes = [vp] * 8 + [i, i] + [f] * 10 + [i, f, i, f, vp, i, i, i]
    for fn in (lib.hostcheck_avg_mean, lib.hostcheck_avg_postpre, lib.hostcheck_avg_mstdp, lib.hostcheck_avg_mstdpet):
        fn.restype = C.c_int
    return lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("K", (1, 2, 31, 32, 33, 255, 256))
def test_ring_mean_equals_torch_mean(host, K):
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(100 + K)
    for E in (1, 5, 31, 32, 33, 1073):
        # values of mixed sign and magnitude, a third of them zero: every add and the division round
        buf = (torch.randn(K, E, generator=g) * torch.exp(3.0 * torch.randn(K, E, generator=g))) * (torch.rand(K, E, generator=g) > 0.33)
        buf = buf.contiguous()
        out = torch.empty(E)
        assert host.hostcheck_avg_mean(_p(buf), K, E, _p(out)) == 0
        want = torch.mean(buf, 0)
        assert torch.equal(out, want), (K, E, int((out != want).sum()))
        assert torch.equal(want, torch.sum(buf, 0) / K)


def _bounds(rule):
    lo, hi = rule._bounds()
    return int(lo is not None), lo or 0.0, int(hi is not None), hi or 0.0


def _bodies(host, monkeypatch):
    """network/host_path.py's three rule functions replaced by the hostcheck bodies (which finish with decay and clamp themselves; the
    clamp _update_mcc still applies behind the reward rules is idempotent, the cases' decay factor is 1)."""
    from bindsnet_amd.network import host_path

    def u8(t):
        return t.to(torch.uint8).contiguous()

    def postpre(rule, W, s_src, x_src, s_tgt, x_tgt, dt):
        i0, i1 = rule._avg_indices()
        assert host.hostcheck_avg_postpre(_p(W), _p(u8(s_src)), _p(x_src.contiguous()), _p(u8(s_tgt)), _p(x_tgt.contiguous()), s_src.shape[0],
                                          W.shape[0], W.shape[1], float(rule.nu[0]), float(rule.nu[1]), dt, float(rule.decay), *_bounds(rule),
                                          int(rule.reduction is torch.squeeze), _p(rule.average_buffer_pre), _p(rule.average_buffer_post),
                                          rule.average_update, int(bool(rule.continues_update)), i0, i1) == 0
        rule._avg_advance()

    def mstdp(rule, W, src_s, tgt_s, kwargs):
        rule._ensure_state()
        r = kwargs["reward"]
        rvec = r.reshape(-1).float().contiguous() if isinstance(r, torch.Tensor) and r.numel() > 1 else None
        dp, dm = rule._decays()
        assert host.hostcheck_avg_mstdp(_p(W), _p(rule.p_plus), _p(rule.p_minus), _p(rule._s_src_prev), _p(rule._s_tgt_prev), _p(u8(src_s)),
                                        _p(u8(tgt_s)), src_s.shape[0], W.shape[0], W.shape[1], 0.0 if rvec is not None else float(r), _p(rvec),
                                        float(rule.nu[0]), float(kwargs.get("a_plus", 1.0)), float(kwargs.get("a_minus", -1.0)), dp, dm,
                                        float(rule.decay), *_bounds(rule), int(rule.reduction is torch.squeeze), _p(rule.average_buffer),
                                        rule.average_update, int(bool(rule.continues_update)), rule._avg_indices()[0]) == 0
        rule._avg_advance()

    def mstdpet(rule, W, dt, src_s, tgt_s, kwargs):
        rule._ensure_state()
        dp, dm, de = rule._decays()
        assert host.hostcheck_avg_mstdpet(_p(W), _p(rule.eligibility_trace), _p(rule.p_plus), _p(rule.p_minus), _p(rule._s_src_prev),
                                          _p(rule._s_tgt_prev), _p(u8(src_s)), _p(u8(tgt_s)), W.shape[0], W.shape[1], float(kwargs["reward"]),
                                          float(rule.nu[0]), dt, float(kwargs.get("a_plus", 1.0)), float(kwargs.get("a_minus", -1.0)), dp, dm,
                                          de, float(rule.tc_e_trace), float(rule.decay), *_bounds(rule), _p(rule.average_buffer),
                                          rule.average_update, int(bool(rule.continues_update)), rule._avg_indices()[0]) == 0
        rule._avg_advance()

    monkeypatch.setattr(host_path, "_postpre_mcc", postpre)
    monkeypatch.setattr(host_path, "_mstdp", mstdp)
    monkeypatch.setattr(host_path, "_mstdpet", mstdpet)


@pytest.mark.parametrize("case", sorted(AC.CASES))
def test_fixture_case_with_the_kernel_bodies(host, monkeypatch, case):
    _bodies(host, monkeypatch)
    NS = ns()
    AC.assert_same(case, AC.run(NS, AC.build(NS, case), case), AC.gold(case, HERE), "kernel bodies on the host")
