"""The batch reductions' kernel arithmetic on the HOST: tests/hostcheck/reduction_host.hip compiles the __host__ __device__ bodies the
update kernels run (csrc/snn_order.hpp BatchReduce / batch_sum<R>, snn_synparams.hpp, snn_average.hpp, snn_half.hpp) with hipcc (no
GPU needed) and drives them element by element, as the kernels' threads do.

  * the reduction bodies against torch.sum / B, torch.amax and torch.amin for B in {1, 2, 3, 31, 32, 33, 255, 256} and E in {1, 5, 31,
    32, 33, 1073}: every column class of ATen's sum(dim=0); inputs with exact zeros, all-negative columns, and -- through the
    accumulator the event-driven kernels use -- columns visited in a subset of the samples only, the others being zero terms;
  * the dense (scalar and per-synapse constants), local, convnd, conv2d-apply, half-precision and averaged update bodies, one
    connection.update() per call, against every update-level fixture case (reference-generated, tests/reduction_cases.py), in place of
    the host path's torch statements."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import reduction_cases as RC
from test_reduction_host import HERE, ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MODES = {"sum": 0, "mean": 1, "amax": 2, "amin": 3}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libreductionhost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "reduction_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    lib.hostcheck_reduce_all.argtypes = [vp, i, C.c_long, i, vp]
    lib.hostcheck_reduce_events.argtypes = [vp, vp, i, C.c_long, i, vp]
    lib.hostcheck_dense_update.argtypes = [vp] * 5 + [i, i, i, i, f, f, i, f, f, i, f, i, f, f, vp, vp, i]
    lib.hostcheck_conv_apply.argtypes = [vp, vp, i, C.c_long, i, f, f, f, i, f, i, f, i]
    lib.hostcheck_local_postpre.argtypes = [vp] * 6 + [i] * 6 + [f, f, f, i, f, i, f, i]
    lib.hostcheck_convnd_postpre.argtypes = [vp] * 6 + [i] * 5 + [f, f, f, i, f, i, f, i]
    lib.hostcheck_avg_postpre_red.argtypes = [vp] * 5 + [i, i, i, f, f, f, f, i, f, i, f, i, vp, vp, i, i, i, i, i]
    lib.hostcheck_avg_mstdp_red.argtypes = [vp] * 7 + [i, i, i, f, vp, f, f, f, f, f, f, i, f, i, f, i, vp, i, i, i, i]
    lib.hostcheck_half_postpre_red.argtypes = [vp, i] + [vp] * 4 + [i, i, i, f, f, i, f, f, i, f, i, f, i]
    for name in ("reduce_all", "reduce_events", "dense_update", "avg_postpre_red", "avg_mstdp_red", "half_postpre_red", "conv_apply", "local_postpre", "convnd_postpre"):
        getattr(lib, "hostcheck_" + name).restype = C.c_int
    return lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _same(a, b):
    """Equal values; zeros of either sign are equal (the sign of a zero result is not defined for amax / amin)."""
    return torch.equal(a + 0.0, b + 0.0)


def _want(buf, red):
    return {"mean": lambda: torch.sum(buf, 0) / buf.shape[0], "amax": lambda: torch.amax(buf, 0), "amin": lambda: torch.amin(buf, 0)}[red]()


@pytest.mark.parametrize("B", (1, 2, 3, 31, 32, 33, 255, 256))
def test_reduction_bodies_equal_torch(host, B):
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(300 + B)
    for E in (1, 5, 31, 32, 33, 1073):
        # values of mixed sign and magnitude, a third of them exact zeros; every fourth column all-negative
        buf = (torch.randn(B, E, generator=g) * torch.exp(3.0 * torch.randn(B, E, generator=g))) * (torch.rand(B, E, generator=g) > 0.33)
        buf[:, ::4] = -buf[:, ::4].abs() - 1e-3
        buf = buf.contiguous()
        # the same values visited in a subset of the samples only: what is not visited is a zero term
        visit = (torch.rand(B, E, generator=g) < 0.5).to(torch.uint8).contiguous()
        sparse = (buf * visit).contiguous()
        for red in RC.TESTED:
            out = torch.empty(E)
            assert host.hostcheck_reduce_all(_p(buf), B, E, MODES[red], _p(out)) == 0
            want = _want(buf, red)
            assert (torch.equal(out, want) if red == "mean" else _same(out, want)), (red, B, E, int((out != want).sum()))
            if red == "mean":
                assert torch.equal(want, torch.mean(buf, 0)), (B, E)
            # (only the sum's order depends on the column class, and the dense kernel's classes are ATen's from eight columns on and
            #  below eight terms; the extremes and the zero they fold in are checked at every size)
            if red != "mean" or E >= 8 or B < 8:
                assert host.hostcheck_reduce_events(_p(sparse), _p(visit), B, E, MODES[red], _p(out)) == 0
                want = _want(sparse, red)
                assert (torch.equal(out, want) if red == "mean" else _same(out, want)), ("events", red, B, E, int((out != want).sum()))
        out = torch.empty(E)
        assert host.hostcheck_reduce_all(_p(buf), B, E, MODES["sum"], _p(out)) == 0 and torch.equal(out, torch.sum(buf, 0))
    assert host.hostcheck_reduce_all(_p(buf), B, E, 4, _p(out)) == -1


def test_extremes_propagate_nan_as_torch_does(host):
    buf = torch.tensor([[1.0, float("nan"), -2.0, 0.5], [float("nan"), 3.0, -1.0, 0.25], [2.0, -1.0, -3.0, float("nan")]]).contiguous()
    visit = torch.tensor([[1, 1, 1, 0], [1, 0, 1, 1], [0, 1, 0, 1]], dtype=torch.uint8).contiguous()
    sparse = torch.where(visit.bool(), buf, torch.zeros(())).contiguous()
    for red in ("amax", "amin"):
        out = torch.empty(4)
        assert host.hostcheck_reduce_all(_p(buf), 3, 4, MODES[red], _p(out)) == 0
        assert torch.equal(torch.isnan(out), torch.tensor([True, True, False, True])) and out[2] == _want(buf, red)[2]
        assert host.hostcheck_reduce_events(_p(sparse), _p(visit), 3, 4, MODES[red], _p(out)) == 0
        want = _want(sparse, red)
        assert torch.equal(torch.isnan(out), torch.isnan(want)) and _same(torch.nan_to_num(out), torch.nan_to_num(want))


def _bounds(rule):
    lo, hi = rule._bounds()
    return int(lo is not None), lo or 0.0, int(hi is not None), hi or 0.0


def _bodies(host, monkeypatch):
    """network/host_path.py's rule functions replaced by the hostcheck bodies (which finish with decay and clamp themselves; the clamp
    the host path still applies behind them is idempotent, the cases' decay factor is 1)."""
    from bindsnet_amd.learning import _descriptor, learning as rules
    from bindsnet_amd.network import host_path

    def u8(t):
        return t.to(torch.uint8).contiguous()

    def mode_of(rule):
        return MODES[_descriptor.reduce_of(rule, rule.source.batch_size)]

    def dense_call(rule, W, mode, s_src, x_src, s_tgt, x_tgt, nu0, nu1, use_dt, dt, decay, reward=0.0, rvec=None):
        """Rates and bounds as the ops hand them to the C ABI: scalars, or -- tensors of more than one element -- an snn_synparams."""
        lo, hi = rule._bounds(tensors=True)
        nu0, nu1, lo, hi, sp, _keep = _descriptor.syn_params(W.shape[0], W.shape[1], W.device, nu0, nu1, lo, hi)
        bounds = (int(lo is not None), lo or 0.0, int(hi is not None), hi or 0.0)
        assert host.hostcheck_dense_update(_p(W), _p(u8(s_src)), _p(x_src.contiguous()), _p(u8(s_tgt)), _p(x_tgt.contiguous()), s_src.shape[0],
                                           W.shape[0], W.shape[1], mode, nu0, nu1, int(use_dt), dt, decay, *bounds, reward, _p(rvec),
                                           None if sp is None else C.addressof(sp), mode_of(rule)) == 0

    def reward_of(kwargs):
        r = kwargs["reward"]
        rvec = r.reshape(-1).float().contiguous() if isinstance(r, torch.Tensor) and r.numel() > 1 else None
        return (0.0 if rvec is not None else float(r)), rvec

    def postpre_mcc(rule, W, s_src, x_src, s_tgt, x_tgt, dt):
        B = s_src.shape[0]
        if getattr(rule, "average_update", 0):
            i0, i1 = rule._avg_indices()
            assert host.hostcheck_avg_postpre_red(_p(W), _p(u8(s_src)), _p(x_src.contiguous()), _p(u8(s_tgt)), _p(x_tgt.contiguous()), B,
                                                  W.shape[0], W.shape[1], float(rule.nu[0]), float(rule.nu[1]), dt, float(rule.decay),
                                                  *_bounds(rule), int(rule.reduction is torch.squeeze), _p(rule.average_buffer_pre),
                                                  _p(rule.average_buffer_post), rule.average_update, int(bool(rule.continues_update)), i0, i1,
                                                  mode_of(rule)) == 0
            rule._avg_advance()
        elif W.dtype != torch.float32:
            bits = W.view(torch.int16)
            assert host.hostcheck_half_postpre_red(_p(bits), 1 if W.dtype == torch.float16 else 2, _p(u8(s_src)), _p(x_src.contiguous()),
                                                   _p(u8(s_tgt)), _p(x_tgt.contiguous()), B, W.shape[0], W.shape[1], float(rule.nu[0]),
                                                   float(rule.nu[1]), 1, dt, float(rule.decay), *_bounds(rule), mode_of(rule)) == 0
        else:
            dense_call(rule, W, 0, s_src, x_src, s_tgt, x_tgt, float(rule.nu[0]), float(rule.nu[1]), True, dt, float(rule.decay))

    def mstdp(rule, W, src_s, tgt_s, kwargs):
        rule._ensure_state()
        reward, rvec = reward_of(kwargs)
        dp, dm = rule._decays()
        decay = float(getattr(rule, "decay", getattr(rule, "weight_decay", 1.0)))
        if getattr(rule, "average_update", 0):
            assert host.hostcheck_avg_mstdp_red(_p(W), _p(rule.p_plus), _p(rule.p_minus), _p(rule._s_src_prev), _p(rule._s_tgt_prev),
                                                _p(u8(src_s)), _p(u8(tgt_s)), src_s.shape[0], W.shape[0], W.shape[1], reward, _p(rvec),
                                                float(rule.nu[0]), float(kwargs.get("a_plus", 1.0)), float(kwargs.get("a_minus", -1.0)), dp, dm,
                                                decay, *_bounds(rule), int(rule.reduction is torch.squeeze), _p(rule.average_buffer),
                                                rule.average_update, int(bool(rule.continues_update)), rule._avg_indices()[0], mode_of(rule)) == 0
            rule._avg_advance()
            return
        dense_call(rule, W, 1, rule._s_src_prev, rule.p_plus, rule._s_tgt_prev, rule.p_minus, float(rule.nu[0]), 0.0, False, 1.0, decay,
                   reward, rvec)
        host_path._advance_p(rule, dp, dm, src_s, tgt_s, kwargs)

    def update_dense(conn, kwargs, mask):
        rule = conn.update_rule
        B = conn.source.batch_size
        W = conn.w.data
        rule._check_reduction()
        src_s, tgt_s = conn.source.s.view(B, -1), conn.target.s.view(B, -1)
        if isinstance(rule, rules.MSTDP):
            return mstdp(rule, W, src_s.float(), tgt_s.float(), kwargs)
        mode = 0 if isinstance(rule, rules.PostPre) else 2 if isinstance(rule, rules.Hebbian) else 3
        dense_call(rule, W, mode, src_s, conn.source.x.view(B, -1), tgt_s, conn.target.x.view(B, -1), rule._nu(0), rule._nu(1),
                   False, 1.0, float(rule.weight_decay))

    def update_conv2d(conn, kwargs, mask):
        """Phase 1 (the per-sample partial sums, which no reduction touches) by the host path's own bmm; phase 2 by the apply body."""
        from bindsnet_amd.utils import im2col_indices
        rule = conn.update_rule
        rule._check_reduction()
        W = conn.w.data
        Cout, _, kh, kw = W.shape
        B = conn.source.batch_size
        src_x = im2col_indices(conn.source.x.view(B, *conn.source.shape), kh, kw, padding=conn.padding, stride=conn.stride)
        src_s = im2col_indices(conn.source.s.view(B, *conn.source.shape).float(), kh, kw, padding=conn.padding, stride=conn.stride)
        tgt_x, tgt_s = conn.target.x.view(B, Cout, -1), conn.target.s.view(B, Cout, -1).float()
        part = torch.stack([torch.bmm(tgt_x, src_s.permute(0, 2, 1)), torch.bmm(tgt_s, src_x.permute(0, 2, 1))]).contiguous()
        mode = 0 if isinstance(rule, rules.PostPre) else 1 if isinstance(rule, rules.Hebbian) else 2
        assert host.hostcheck_conv_apply(_p(W), _p(part), B, W.numel(), mode, float(rule.nu[0]), float(rule.nu[1]), float(rule.weight_decay),
                                         *_bounds(rule), mode_of(rule)) == 0

    def postpre_local(conn, rule):
        B, W = conn.source.batch_size, conn.w.data
        src = conn.src.to(torch.int32).contiguous()
        assert host.hostcheck_local_postpre(_p(W), _p(src), _p(u8(conn.source.s.reshape(B, -1))), _p(conn.source.x.reshape(B, -1).contiguous()),
                                            _p(u8(conn.target.s.reshape(B, -1))), _p(conn.target.x.reshape(B, -1).contiguous()), B,
                                            src.shape[0], conn.n_filters * src.shape[1], src.shape[1], src.shape[2], conn.source.n,
                                            float(rule.nu[0]), float(rule.nu[1]), float(rule.weight_decay), *_bounds(rule), mode_of(rule)) == 0

    def postpre_convnd(conn, rule):
        B, W = conn.source.batch_size, conn.w.data
        tab = conn.pp_src.to(torch.int32).contiguous()
        assert host.hostcheck_convnd_postpre(_p(W), _p(tab), _p(u8(conn.source.s.reshape(B, -1))), _p(conn.source.x.reshape(B, -1).contiguous()),
                                             _p(u8(conn.target.s.reshape(B, -1))), _p(conn.target.x.reshape(B, -1).contiguous()), B,
                                             W.shape[0], tab.shape[0], tab.shape[1], conn.source.n, float(rule.nu[0]), float(rule.nu[1]),
                                             float(rule.weight_decay), *_bounds(rule), mode_of(rule)) == 0

    monkeypatch.setattr(host_path, "_postpre_mcc", postpre_mcc)
    monkeypatch.setattr(host_path, "_mstdp", mstdp)
    from bindsnet_amd.network import topology
    monkeypatch.setattr(topology._DenseConnection, "_host_update", lambda self, kwargs, mask: update_dense(self, kwargs, mask))
    monkeypatch.setattr(topology.Conv2dConnection, "_host_update", lambda self, kwargs, mask: update_conv2d(self, kwargs, mask))
    monkeypatch.setattr(topology._LocalConnectionND, "_host_postpre", lambda self, rule: postpre_local(self, rule))
    monkeypatch.setattr(topology._ConvNdConnection, "_host_postpre", lambda self, rule: postpre_convnd(self, rule))


BODY_CASES = sorted(RC.CASES)


@pytest.mark.parametrize("case", BODY_CASES)
def test_update_level_fixture_with_the_kernel_bodies(host, monkeypatch, case):
    _bodies(host, monkeypatch)
    _, want = RC.gold(case, HERE)
    RC.assert_same(case, RC.run_updates(RC.build(ns(), case), case), want, "kernel bodies on the host")
