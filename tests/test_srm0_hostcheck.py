"""The SRM0Nodes / Rmax kernels' arithmetic on the HOST: tests/hostcheck/srm0_host.hip compiles the __host__ __device__ bodies of
csrc/snn_common.hpp with hipcc (no GPU needed) and drives them element by element, as the kernels' threads do, from what the
reference-generated fixtures recorded.

  * the SRM0 body with the fixture's recorded draws and the host's expf: raster, per-step v, refrac_count and trace bit for bit, s_prob
    within the device bound (two 1-ulp exponentials: 8 * 2^-24);
  * the Rmax body with the fixture's recorded per-step s, s_prob and source trace: eligibility_trace and w bit for bit -- the
    operation order without any exponential in the way;
  * the stream walk from the fixture's entry state: the recorded draws and the exit state."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cases
import srm0_cases as SC
from test_srm0_host import _bits, build, gold, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
f32, u8 = np.float32, np.uint8
DELTA_P = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    from bindsnet_amd._lib import LifParams
    out = str(tmp_path_factory.mktemp("hostcheck") / "libsrm0host.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "srm0_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    lib.hostcheck_srm0_run.argtypes = [vp] * 6 + [i, i, i, C.POINTER(LifParams), f, f, f] + [vp] * 6
    lib.hostcheck_srm0_run.restype = None
    lib.hostcheck_rmax_run.argtypes = [vp] * 5 + [i, i, i] + [f] * 6 + [i, f, i, f, vp]
    lib.hostcheck_rmax_run.restype = None
    lib.hostcheck_stream_walk.argtypes = [vp, vp, C.c_long, vp]
    lib.hostcheck_stream_walk.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


DIRECT = sorted(n for n, c in SC.CASES.items() if c["graph"] in ("direct", "two"))


@pytest.mark.parametrize("name", DIRECT)
def test_srm0_body_reproduces_reference_fixture(host, name):
    c, g = SC.CASES[name], gold(name)
    T, B = c["T"], c["B"]
    net = build(name)                                   # this package's layers: the source of the parameters and initial state
    for L in SC.srm0_layers(name):
        Y = net.layers[L]
        Y.set_batch_size(B)
        n = Y.n
        for r in range(c["n_in"]):
            Y.reset_state_variables()
            v, rc, x = (getattr(Y, k).numpy().astype(f32).copy() for k in ("v", "refrac_count", "x"))
            s = np.zeros((B, n), u8)
            cur = np.ascontiguousarray(SC.inputs(name, r)[L])
            u = np.ascontiguousarray(g[f"r{r}_{L}_u"], f32)
            pv = {}
            p = Y._params(pv)
            tv = pv["thresh"].numpy().copy() if "thresh" in pv else None
            dv = pv["decay"].numpy().copy() if "decay" in pv else None
            raster, vrec, prec, rrec = np.zeros((T, B, n), u8), np.zeros((T, B, n), f32), np.zeros((T, B, n), f32), np.zeros((T, B, n), f32)
            host.hostcheck_srm0_run(_p(v), _p(rc), _p(s), _p(x), _p(cur), _p(u), T, B, n, C.byref(p), float(Y.eps_0), float(Y.rho_0),
                                    float(Y.d_thresh), _p(tv), _p(dv), _p(raster), _p(vrec), _p(prec), _p(rrec))
            want = cases.unpack(g[f"r{r}_{L}_raster"], raster.shape)
            assert 0 < want.sum() < want.size
            assert np.array_equal(raster, want), f"case {name} input {r}: {L} raster differs"
            same(vrec, g[f"r{r}_{L}_vrec"], f"case {name} input {r}: per-step v of {L}")
            same(rc, g[f"r{r}_{L}_rc"], f"case {name} input {r}: refrac_count of {L}")
            same(x, g[f"r{r}_{L}_x"], f"case {name} input {r}: trace of {L}")
            d = np.abs(prec.astype(np.float64) - g[f"r{r}_{L}_prec"].astype(np.float64)).max()
            print(f"case {name} input {r} layer {L}: largest |s_prob - reference| = {d:.3g} (bound {DELTA_P:.3g})")
            assert d <= DELTA_P
            assert np.isfinite(rrec).all() and (rrec > 0).all()


@pytest.mark.parametrize("name", SC.RULE_CASES)
def test_rmax_body_reproduces_reference_fixture(host, name):
    c, g = SC.CASES[name], gold(name)
    T = c["T"]
    net = build(name)
    conn = net.connections[("X", "Y")]
    rule = conn.update_rule
    W = conn.w.detach().numpy().astype(f32).copy()
    same(W, g["w0"], "initial weights")
    e = np.zeros_like(W)
    mask = conn.mask.numpy().astype(u8).copy() if getattr(conn, "mask", None) is not None else None
    lo, hi = rule._bounds()
    for r in range(c["n_in"]):
        s = np.ascontiguousarray(cases.unpack(g[f"r{r}_Y_raster"], (T, c["n"])), u8)
        p = np.ascontiguousarray(g[f"r{r}_Y_prec"].reshape(T, c["n"]), f32)
        x = np.ascontiguousarray(g[f"r{r}_rx"], f32)
        host.hostcheck_rmax_run(_p(W), _p(e), _p(s), _p(p), _p(x), T, c["S"], c["n"], float(c["reward"]), float(rule.nu[0]), float(conn.dt),
                                float(rule.tc_c), float(rule.tc_e_trace), float(rule.weight_decay), int(lo is not None), lo or 0.0,
                                int(hi is not None), hi or 0.0, _p(mask))
        same(e, g[f"r{r}_e"], f"case {name} input {r}: eligibility_trace")
        same(W, g[f"r{r}_w"], f"case {name} input {r}: weights")
    assert np.abs(W - g["w0"]).max() > 1e-2


@pytest.mark.parametrize("name", ["d_b1n24_w0", "d_b3n101_w5", "d_b1n624_w623", "d_b2n313_w0", "d_b5n257_w623", "two"])
def test_stream_walk_reproduces_draws_and_exit_state(host, name):
    from bindsnet_amd import rng
    c, g = SC.CASES[name], gold(name)
    st0 = torch.from_numpy(g["r0_rng0"])
    img = rng.torch_state_to_words(st0).copy()
    mt, pos = img[:624].view(np.uint32).copy(), np.array([int(img[624])], np.int32)
    for t in range(c["T"]):
        for L in SC.srm0_layers(name):
            want = np.ascontiguousarray(g[f"r0_{L}_u"][t].reshape(-1), f32)
            out = np.zeros_like(want)
            host.hostcheck_stream_walk(_p(mt), _p(pos), want.size, _p(out))
            assert np.array_equal(_bits(out), _bits(want)), (name, t, L)
    img[:624], img[624] = mt.view(np.int32), int(pos[0])
    assert torch.equal(rng.words_to_torch_state(img, st0), torch.from_numpy(g["r0_rng1"])) or \
        np.array_equal(rng.torch_state_to_words(rng.words_to_torch_state(img, st0)), rng.torch_state_to_words(torch.from_numpy(g["r0_rng1"])))


@pytest.mark.parametrize("warm", [0, 300, 623, 624])
@pytest.mark.parametrize("count", [5, 303, 623, 624, 626, 1285])
def test_stream_walk_equals_torch_rand_like(host, warm, count):
    """The product's own conversion and walk (srm0_uniform, mt_temper, mt_mix) against torch.rand_like itself: from block position
    "twist first" (a fresh seed, and 624 draws later), mid-block and 623; element counts below, at and above a block."""
    from bindsnet_amd import rng
    torch.manual_seed(17 + warm)
    if warm:
        torch.rand(warm)
    st = torch.get_rng_state()
    img = rng.torch_state_to_words(st).copy()
    mt, pos = img[:624].view(np.uint32).copy(), np.array([int(img[624])], np.int32)
    want = torch.rand_like(torch.empty(count)).numpy()
    after = torch.get_rng_state()
    out = np.zeros(count, f32)
    host.hostcheck_stream_walk(_p(mt), _p(pos), count, _p(out))
    assert np.array_equal(_bits(out), _bits(want))
    img[:624], img[624] = mt.view(np.int32), int(pos[0])
    torch.set_rng_state(rng.words_to_torch_state(img, st))
    a = torch.rand(700)
    torch.set_rng_state(after)
    assert torch.equal(a, torch.rand(700)), "the walked state is not where torch.rand_like leaves the generator"
