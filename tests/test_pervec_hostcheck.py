"""The per-neuron instances of the step kernels on the HOST: tests/hostcheck/pervec_host.hip compiles the __host__ __device__ text of
csrc/snn_common.hpp -- row_of<true> and the update functions that take a neuron's own threshold and decays -- with hipcc (no GPU
needed) and runs it sample by sample, neuron by neuron, as the kernels' threads do.  Every case of tests/pervec_cases.py is stepped
that way against its reference-generated fixture, bit for bit; the currents come from the host path's propagation, the one_spike
draws from torch.multinomial, PostPre from the host path's statement of it.

The source does not compile against a snn_common.hpp whose update functions read their thresholds and decays from the scalar
parameter block only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pervec_cases as PC
from test_pervec_host import check_snapshots, ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KIND = {"mcp": 0, "if": 1, "boosted": 2, "clif": 3, "lif": 4}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    from bindsnet_amd._lib import DcParams, LifParams, PerVec
    out = str(tmp_path_factory.mktemp("hostcheck") / "libpervechost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "pervec_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp, i = C.c_void_p, C.c_int
    lib.hostcheck_pv_step.argtypes = [i] + [vp] * 6 + [i, i, C.POINTER(LifParams), C.c_float, C.POINTER(PerVec)]
    lib.hostcheck_pv_dc_membrane.argtypes = [vp] * 5 + [i, i, C.POINTER(DcParams), C.POINTER(PerVec)]
    lib.hostcheck_pv_trace.argtypes = [vp, vp, i, i, C.POINTER(LifParams), C.POINTER(PerVec)]
    lib.hostcheck_pv_izh.argtypes = [vp] * 10 + [i, i, C.POINTER(LifParams), C.POINTER(PerVec)]
    for fn in (lib.hostcheck_pv_step, lib.hostcheck_pv_dc_membrane, lib.hostcheck_pv_trace, lib.hostcheck_pv_izh):
        fn.restype = None
    return lib


def _p(t):
    assert t.is_contiguous() and not t.is_cuda
    return C.c_void_p(t.data_ptr())


def _step_layer(host, c, Y, cur, B, n):
    """One timestep of layer Y on the compiled kernel text; the parameters and the vectors are what the device path would launch with."""
    from bindsnet_amd import _lib
    from bindsnet_amd.network import host_path
    pv = {}
    kind = c["kind"]
    if kind in ("dc", "alif"):
        p = Y._dc_params(pv)
        assert pv, "the case has no per-neuron parameter"
        vec = _lib.pervec(pv)
        host.hostcheck_pv_dc_membrane(_p(Y.v), _p(Y.refrac_count), _p(Y.s), _p(Y.theta), _p(cur), B, n, C.byref(p), C.byref(vec))
        if Y.one_spike:
            host_path._one_spike(Y.s.view(B, -1))
        host.hostcheck_pv_trace(_p(Y.s), _p(Y.x), B, n, C.byref(p.lif), C.byref(vec))
        return
    if kind == "izh":
        p = Y._node_params(pv)
        a, b, cc, d = Y._abcd()
        vec = _lib.pervec(pv)
        host.hostcheck_pv_izh(_p(Y.v), _p(Y.u), _p(Y.s), _p(Y.x), _p(cur), _p(a), _p(b), _p(cc), _p(d), _p(Y._St()), B, n, C.byref(p), C.byref(vec))
        return
    aux, aux_decay = None, 0.0
    if kind == "lif":
        p = Y._lif_params(pv)
    elif kind == "mcp":
        p = Y._node_params(pv)
    else:
        p = Y._params(pv)
        if kind == "clif":
            aux, aux_decay = Y.i, Y._sv("i_decay", pv)
    null = torch.zeros(1)
    vec = _lib.pervec(pv) or _lib.PerVec()
    host.hostcheck_pv_step(KIND[kind], _p(Y.v), _p(getattr(Y, "refrac_count", null) if kind != "mcp" else null), _p(aux if aux is not None else null),
                           _p(Y.s), _p(Y.x), _p(cur), B, n, C.byref(p), aux_decay, C.byref(vec))


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_per_neuron_update_text_reproduces_reference_fixture(host, name):
    from bindsnet_amd import _lib
    from bindsnet_amd.network import host_path
    c = PC.CASES[name]
    T, B, n = c["T"], c["B"], int(np.prod(c["shape"]))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        net = PC.build(ns(), name)
        from test_pervec_host import gold
        PC.load_derived(net, gold(name))
        X, Y = net.layers["X"], net.layers["Y"]
        for layer in (X, Y):
            layer.set_batch_size(B)
        conn, rec = net.connections[("X", "Y")], net.connections.get(("Y", "Y"))
        rule = conn._weight().learning_rule
        snaps = []
        torch.manual_seed(100 + c["seed"])
        for r in range(c["n_in"]):
            inp = torch.from_numpy(PC.inputs(name, r))
            raster = np.zeros((T, B, n), np.uint8)
            xs = torch.zeros(B, PC.N_SRC, dtype=torch.uint8)           # Input.s as the connections see it before the layers step
            for t in range(T):
                cur = torch.zeros(B, *Y.shape)
                cur += host_path._propagate_mcc(conn, xs)
                if rec is not None:
                    cur += host_path._propagate_mcc(rec, Y.s)
                cur = cur.reshape(B, n).contiguous()
                xs = inp[t].contiguous()
                xpv = {}
                xp = _lib.LifParams()
                X._trace_fields(xp, xpv)
                xvec = _lib.pervec(xpv) or _lib.PerVec()
                host.hostcheck_pv_trace(_p(xs), _p(X.x), B, PC.N_SRC, C.byref(xp), C.byref(xvec))
                _step_layer(host, c, Y, cur, B, n)
                if c.get("postpre"):
                    host_path._postpre_mcc(rule, conn._weight().value.data, xs, X.x.view(B, -1), Y.s.view(B, -1), Y.x.view(B, -1), c.get("dt", 1.0))
                raster[t] = Y.s.view(B, n).numpy().astype(np.uint8)
            snaps.append(PC.snapshot(net, name, raster))
            net.reset_state_variables()
    finally:
        torch.set_num_threads(threads)
    check_snapshots(name, snaps)
