"""The node step kernels' arithmetic on the HOST: tests/hostcheck/nodes_host.hip compiles the __host__ __device__ update bodies of
csrc/snn_common.hpp and the lateral-sum accumulator of csrc/snn_order.hpp with hipcc (no GPU needed) and drives them element by
element, term by term, as the kernels' threads do.

  * every direct fixture case of tests/node_cases.py (reference-generated): raster, per-step v, every final state tensor, bit for bit;
  * the Izhikevich lateral sum against torch's own S[:, mask].sum(dim=1): random matrices and masks, EVERY k from 1 to n, for layer
    sizes up to SNN_IZH_MAX_N = 1024 -- the comparison that sets the supported layer size (snnhip.h, _lib.IZH_MAX_N)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import node_cases as NC
from test_nodes_host import _bits, _ns, build, check_snapshots, gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
f32, u8 = np.float32, np.uint8
KIND = {"mcp": 0, "if": 1, "boosted": 2, "clif": 3}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    from bindsnet_amd._lib import LifParams
    out = str(tmp_path_factory.mktemp("hostcheck") / "libnodeshost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "nodes_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.hostcheck_node_run.argtypes = [C.c_int] + [vp] * 6 + [C.c_int, C.c_long, C.POINTER(LifParams), C.c_float, vp, vp]
    lib.hostcheck_node_run.restype = None
    lib.hostcheck_lateral.argtypes = [vp, vp, C.c_int, vp]
    lib.hostcheck_lateral.restype = None
    lib.hostcheck_izh_run.argtypes = [vp] * 10 + [C.c_int] * 3 + [C.POINTER(LifParams), vp, vp]
    lib.hostcheck_izh_run.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


DIRECT = sorted(n for n, c in NC.CASES.items() if c["graph"] == "direct")


@pytest.mark.parametrize("name", DIRECT)
def test_update_bodies_reproduce_reference_fixture(host, name):
    """The kernels' per-element text over a whole fixture case: what a GPU run of the case computes, without the GPU."""
    c = NC.CASES[name]
    T, B, n = c["T"], c["B"], c["n"]
    net = build(name)                                   # this package's layer: the source of the parameters and initial state
    Y = net.layers["Y"]
    Y.set_batch_size(B)                                 # (Network.run does this when it sees the first input)
    snaps = []
    for r in range(c["n_in"]):
        st = {k: getattr(Y, k).detach().numpy().astype(f32).copy() for k in NC.STATE if isinstance(getattr(Y, k, None), torch.Tensor)}
        s = np.zeros((B, n), u8)
        cur = NC.inputs(name, r)["Y"].copy()
        raster, vrec = np.zeros((T, B, n), u8), np.zeros((T, B, n), f32)
        if c["kind"] == "izh":
            a, b, cc, d = (getattr(Y, k).numpy().astype(f32).copy() for k in "abcd")
            St = np.ascontiguousarray(Y.S.numpy().T, f32)
            p = Y._node_params()
            host.hostcheck_izh_run(_p(st["v"]), _p(st["u"]), _p(s), _p(st["x"]), _p(cur), _p(a), _p(b), _p(cc), _p(d), _p(St), B, n, T,
                                   C.byref(p), _p(raster), _p(vrec))
        else:
            p = Y._node_params() if c["kind"] == "mcp" else Y._params()
            null = np.zeros(1, f32)
            host.hostcheck_node_run(KIND[c["kind"]], _p(st["v"]), _p(st.get("refrac_count", null)), _p(st.get("i", null)), _p(s), _p(st["x"]),
                                    _p(cur), T, B * n, C.byref(p), float(getattr(Y, "i_decay", 0.0)), _p(raster), _p(vrec))
        snaps.append(dict(raster=raster, vrec=vrec, **st))
    check_snapshots(name, snaps)


def _lateral_case(host, n, masks_per_k, seed, signed):
    rng = np.random.default_rng(seed)
    S = rng.random((n, n), dtype=f32)
    if signed:                                          # the mixed regime: excitatory columns 0.5 * rand, inhibitory -rand
        S[:, n - n // 5:] *= -1
    St = np.ascontiguousarray(S.T)
    S_t = torch.from_numpy(S)
    out = np.zeros(n, f32)
    for k in range(1, n + 1):
        for _ in range(masks_per_k):
            mask = np.zeros(n, u8)
            mask[rng.choice(n, k, replace=False)] = 1
            host.hostcheck_lateral(_p(St), _p(mask), n, _p(out))
            want = S_t[:, torch.from_numpy(mask).bool()].sum(dim=1).numpy()
            bad = np.flatnonzero(_bits(out) != _bits(want))
            assert bad.size == 0, f"n = {n}, k = {k}: {bad.size} of {n} sums differ from torch (first rows {bad[:5]})"


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 100, 127, 200])
def test_lateral_sum_equals_torch_for_every_k(host, n):
    _lateral_case(host, n, 3, 100 + n, signed=n % 2 == 0)


@pytest.mark.parametrize("n", [257, 512, 640, 1000, 1024])
def test_lateral_sum_equals_torch_up_to_the_supported_size(host, n):
    """Every k from 1 to n at the sizes up to SNN_IZH_MAX_N: past k = 512 the 16-term flushes of ATen's cascade are reached."""
    from bindsnet_amd import _lib
    assert n <= _lib.IZH_MAX_N == 1024
    _lateral_case(host, n, 1, 200 + n, signed=True)


def test_lateral_sum_at_one_thread(host):
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _lateral_case(host, 300, 1, 77, signed=True)
    finally:
        torch.set_num_threads(n)


def test_header_bound_matches_the_binding():
    from bindsnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snnhip.h")).read()
    assert f"#define SNN_IZH_MAX_N {_lib.IZH_MAX_N}\n" in hdr
