"""tests/hostcheck/synparams_host.hip as a Python object: compiles the __host__ __device__ bodies of csrc/snn_synparams.hpp with hipcc
(no GPU needed) and drives them on CPU tensors with the argument conventions of bindsnet_amd.ops -- rates and bounds as floats, None
or tensors that broadcast against [S, N].  Used by tests/test_synparams_hostcheck.py and as the reference of the device sweep in
tests/test_gpu_synparams.py."""
import ctypes as C
import os
import shutil
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MODES = {"postpre": 0, "mstdp": 1, "hebbian": 2, "wdpostpre": 3}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class HostLib:
    def __init__(self, workdir):
        from bindsnet_amd import _lib
        out = os.path.join(str(workdir), "libsynhost.so")
        src = os.path.join(ROOT, "tests", "hostcheck", "synparams_host.hip")
        subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src,
                        "-o", out], check=True, capture_output=True, timeout=600)
        self.lib = C.CDLL(out)
        vp, i, f, sp = C.c_void_p, C.c_int, C.c_float, C.POINTER(_lib.SynParams)
        self.lib.hostcheck_syn_update.argtypes = [i] + [vp] * 5 + [i, i, i, f, f, i, f, f, i, f, i, f, sp, f, vp]
        self.lib.hostcheck_syn_mstdpet.argtypes = [vp] * 6 + [i, i] + [f] * 6 + [i, f, i, f, sp]
        self.lib.hostcheck_syn_normalize.argtypes = [vp, vp, vp, i, i]
        for fn in (self.lib.hostcheck_syn_update, self.lib.hostcheck_syn_mstdpet, self.lib.hostcheck_syn_normalize):
            fn.restype = i

    @staticmethod
    def _consts(W, nu0, nu1, wmin, wmax):
        from bindsnet_amd import _lib
        from bindsnet_amd.learning._descriptor import syn_params
        nu0, nu1, lo, hi, sp, keep = syn_params(W.shape[0], W.shape[1], "cpu", nu0, nu1, wmin, wmax)
        sp = sp if sp is not None else _lib.SynParams()
        return nu0, nu1, (int(lo is not None), lo or 0.0, int(hi is not None), hi or 0.0), sp, keep

    def update(self, mode, W, s_src, x_src, s_tgt, x_tgt, nu0, nu1=0.0, use_dt=False, dt=1.0, decay=1.0, wmin=None, wmax=None, reward=0.0,
               reward_vec=None):
        """One update of W [S, N] (in place) on [B, S] / [B, N] factors; for "mstdp" x_src / x_tgt are p_plus / p_minus and s_* the previous spikes."""
        B = s_src.shape[0]
        nu0, nu1, bounds, sp, keep = self._consts(W, nu0, nu1, wmin, wmax)
        s_src, s_tgt = s_src.to(torch.uint8).contiguous(), s_tgt.to(torch.uint8).contiguous()
        x_src, x_tgt = x_src.contiguous(), x_tgt.contiguous()
        rc = self.lib.hostcheck_syn_update(MODES[mode], _p(W), _p(s_src), _p(x_src), _p(s_tgt), _p(x_tgt), B, W.shape[0], W.shape[1], nu0, nu1,
                                           int(use_dt), dt, decay, *bounds, C.byref(sp), reward, _p(reward_vec))
        assert rc == 0, rc

    def mstdpet(self, W, e_trace, p_plus, p_minus, s_src_prev, s_tgt_prev, reward, nu0, dt, decay_e, tc_e, wdecay=1.0, wmin=None, wmax=None):
        nu0, _, bounds, sp, keep = self._consts(W, nu0, 0.0, wmin, wmax)
        p_plus, p_minus = p_plus.contiguous(), p_minus.contiguous()
        s_src_prev, s_tgt_prev = s_src_prev.to(torch.uint8).contiguous(), s_tgt_prev.to(torch.uint8).contiguous()
        rc = self.lib.hostcheck_syn_mstdpet(_p(W), _p(e_trace), _p(p_plus), _p(p_minus), _p(s_src_prev), _p(s_tgt_prev),
                                            W.shape[0], W.shape[1], reward, nu0, dt, decay_e, tc_e, wdecay, *bounds, C.byref(sp))
        assert rc == 0, rc

    def normalize(self, W, norm, use_abs):
        """W [S, N] (in place) to the per-target totals `norm` ([N] or [1, N]); the column sums are torch's."""
        colsum = (W.abs() if use_abs else W).sum(0).contiguous()
        norm = norm.reshape(-1).float().contiguous()
        assert self.lib.hostcheck_syn_normalize(_p(W), _p(colsum), _p(norm), W.shape[0], W.shape[1]) == 0
