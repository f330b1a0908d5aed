"""The conversion kernels' arithmetic on the HOST: tests/hostcheck/conversion_host.hip compiles the __host__ __device__ bodies of
csrc/snn_conversion.hpp with hipcc (no GPU needed) and drives them element by element, as the kernels do.

  * the step of SubtractiveResetIFNodes against torch's own expressions (the reference's forward(), written out) for every N from 1
    to 130, with and without a lower bound, a refractory period, dt = 0.5, every trace mode and `summed`;
  * the step fixtures of tests/conversion_cases.py (reference-generated) with these bodies in place of the host path;
  * the gather's index rule against s.permute(dims) for every permutation of three dimensions (and of two, and of one) and against
    F.pad for random paddings, with and without accumulate; geometries that would read out of bounds are refused;
  * the pass-through byte against x != 0."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conversion_cases as CC
from test_conversion_host import check_snapshots, gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libconversionhost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "conversion_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp, three = C.c_void_p, C.POINTER(C.c_int)
    lib.hostcheck_sif_run.argtypes = [vp] * 6 + [C.c_int, C.c_long, vp, vp, vp, vp]
    lib.hostcheck_sif_run.restype = None
    lib.hostcheck_pass.argtypes = [vp, vp, C.c_long]
    lib.hostcheck_pass.restype = None
    lib.hostcheck_gather.argtypes = [vp, vp, C.c_long, C.c_long] + [three] * 4 + [C.c_int]
    lib.hostcheck_gather.restype = C.c_int
    return lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _params(thresh, refrac, dt, lbound, traces, additive, trace_decay, trace_scale):
    from bindsnet_amd import _lib
    p = _lib.LifParams()
    p.thresh, p.refrac, p.dt = thresh, refrac, dt
    p.has_lbound, p.lbound = int(lbound is not None), 0.0 if lbound is None else lbound
    p.traces, p.traces_additive, p.trace_decay, p.trace_scale = int(traces), int(additive), trace_decay, trace_scale
    return p


def _sif(host, cur, p, summed, scale_vec=None, v0=0.0):
    T, n = cur.shape
    v, rc, x = torch.full((n,), v0), torch.zeros(n), torch.zeros(n)
    s, raster, vrec = torch.zeros(n, dtype=torch.uint8), torch.zeros(T, n, dtype=torch.uint8), torch.zeros(T, n)
    sm = torch.zeros(n) if summed else None
    host.hostcheck_sif_run(_p(v), _p(rc), _p(s), _p(x), _p(sm), _p(cur), T, n, C.byref(p), _p(scale_vec), _p(raster), _p(vrec))
    return dict(v=v, rc=rc, x=x, summed=sm, raster=raster, vrec=vrec)


def _torch_sif(cur, thresh, refrac, dt, lbound, traces, additive, trace_decay, trace_scale, summed, v0=0.0):
    """conversion/nodes.py:81-97 and nodes.py:96-107 in torch's own calls."""
    T, n = cur.shape
    v, rc, x, sm = torch.full((n,), v0), torch.zeros(n), torch.zeros(n), torch.zeros(n)
    raster, vrec = torch.zeros(T, n, dtype=torch.uint8), torch.zeros(T, n)
    dt, thresh = torch.tensor(dt), torch.tensor(thresh)
    for t in range(T):
        v += (rc == 0).float() * cur[t]
        rc = (rc > 0).float() * (rc - dt)
        s = v >= thresh
        rc.masked_fill_(s, refrac)
        v[s] = v[s] - thresh
        if lbound is not None:
            v.masked_fill_(v < lbound, lbound)
        if traces:
            x *= trace_decay
            if additive:
                x += trace_scale * s.float()
            else:
                x.masked_fill_(s, trace_scale)
        if summed:
            sm += cur[t]
        raster[t], vrec[t] = s, v
    return dict(v=v, rc=rc, x=x, summed=sm if summed else None, raster=raster, vrec=vrec)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))      # bits: -0.0 is not +0.0


def test_step_equals_torch_for_every_n(host):
    gen = torch.Generator().manual_seed(11)
    decay = float(torch.exp(-torch.tensor(1.0) / torch.tensor(8.0)))
    spikes = 0
    for n in range(1, 131):
        mode = n % 4                                   # traces: off, set, additive, additive with a per-neuron scale
        lbound = -0.75 if n % 2 else None
        refrac, dt = (2, 0.5) if n % 3 == 0 else ((3, 1.0) if n % 3 == 1 else (0, 1.0))
        cur = (torch.rand(12, n, generator=gen) * 3 - 1.2).contiguous()          # ordinary floats: nothing here depends on an order
        cur[2] = -1.5
        scale_vec = torch.linspace(0.5, 1.5, n) if mode == 3 else None
        p = _params(1.0, refrac, dt, lbound, mode > 0, mode >= 2, decay, 0.75)
        got = _sif(host, cur, p, summed=n % 5 != 0, scale_vec=scale_vec, v0=0.125)
        want = _torch_sif(cur, 1.0, refrac, dt, lbound, mode > 0, mode >= 2, decay, scale_vec if mode == 3 else 0.75, n % 5 != 0, v0=0.125)
        for k in got:
            if got[k] is None:
                assert want[k] is None
                continue
            assert _same(got[k], want[k]), (n, k)
        spikes += int(got["raster"].sum())
    assert spikes > 1000


@pytest.mark.parametrize("name", list(CC.STEP))
def test_step_fixtures_with_the_kernel_text(host, name):
    g = gold(name)
    c = CC.STEP[name]
    kw = CC.step_layer_kwargs(name)
    decay = float(torch.exp(-torch.tensor(c["dt"]) / torch.tensor(8.0))) if c["traces"] else 0.0
    scale = kw.get("trace_scale", 1.0)
    p = _params(1.0, c["refrac"], c["dt"], c["lbound"], bool(c["traces"]), c["traces"] in ("add", "pv"), decay, 0.0 if isinstance(scale, torch.Tensor) else scale)
    snaps = []
    for r in range(CC.N_IN):
        cur = torch.from_numpy(CC.step_currents(name, r)).reshape(CC.STEP_T, -1).contiguous()
        vec = scale.repeat(c["B"]).contiguous() if isinstance(scale, torch.Tensor) else None
        out = _sif(host, cur, p, summed=c["sum"], scale_vec=vec)
        snap = {"Y_raster": out["raster"].numpy().reshape(CC.STEP_T, c["B"], -1), "Y_v": out["v"].numpy(), "Y_rc": out["rc"].numpy()}
        if c["traces"]:
            snap["Y_x"] = out["x"].numpy()
        if c["sum"]:
            snap["Y_summed"] = out["summed"].numpy()
        snaps.append(snap)
    check_snapshots(name, snaps, g)


def _gather(host, s, arrays, out_shape, prev=None):
    B = s.shape[0]
    out = torch.zeros(B, *out_shape) if prev is None else prev.clone().contiguous()
    s = s.to(torch.uint8).contiguous()
    rc = host.hostcheck_gather(_p(s), _p(out), B, s.numel() // B, *arrays, int(prev is not None))
    assert rc == 0, rc
    return out


def test_every_permutation_equals_torch(host):
    from bindsnet_amd import ops
    gen = torch.Generator().manual_seed(12)
    for shape in ((2, 3, 5), (4, 1, 3), (7,), (3, 4)):
        s = torch.rand(3, *shape, generator=gen) < 0.5
        for dims in itertools.permutations(range(len(shape))):
            arrays, out_shape = ops.permute_geometry(shape, dims)
            want = s.permute(0, *[d + 1 for d in dims]).float()
            assert out_shape == tuple(want.shape[1:])
            assert torch.equal(_gather(host, s, arrays, out_shape), want), (shape, dims)
            prev = torch.rand(3, *out_shape, generator=gen)
            assert torch.equal(_gather(host, s, arrays, out_shape, prev=prev), prev + want), (shape, dims, "accumulate")


def test_padding_equals_torch(host):
    from bindsnet_amd import ops
    rng = np.random.default_rng(13)
    gen = torch.Generator().manual_seed(13)
    for trial in range(40):
        shape = tuple(int(v) for v in rng.integers(1, 7, size=int(rng.integers(2, 4))))
        l, r, t, b = (int(v) for v in rng.integers(0, 4, size=4))
        if trial == 0:
            l = r = t = b = 0
        s = torch.rand(2, *shape, generator=gen) < 0.6
        lead = (0,) * (len(shape) - 2)
        arrays, out_shape = ops.pad_geometry(shape, lead + (t, l), lead + (b, r))
        want = F.pad(s, (l, r, t, b)).float()
        assert out_shape == tuple(want.shape[1:])
        assert torch.equal(_gather(host, s, arrays, out_shape), want), (shape, (l, r, t, b))
        prev = torch.rand(2, *out_shape, generator=gen)
        assert torch.equal(_gather(host, s, arrays, out_shape, prev=prev), prev + want)


def test_unsound_geometries_are_refused(host):
    from bindsnet_amd import ops
    s, out = torch.zeros(1, 30, dtype=torch.uint8), torch.zeros(1, 30)
    good, _ = ops.permute_geometry((2, 3, 5), (2, 0, 1))
    assert host.hostcheck_gather(_p(s), _p(out), 1, 30, *good, 0) == 0
    assert host.hostcheck_gather(_p(s), _p(out), 1, 29, *good, 0) == -1                      # the last element would lie outside the source
    for field, a, value in ((2, 0, 16), (1, 2, 4), (3, 1, 1), (0, 0, 0), (2, 1, -1)):        # a stride, an extent, a cropping offset, an empty output, a negative stride
        arrays, _ = ops.permute_geometry((2, 3, 5), (2, 0, 1))
        arrays[field][a] = value
        assert host.hostcheck_gather(_p(s), _p(out), 1, 30, *arrays, 0) == -1, (field, a, value)


def test_pass_through_byte(host):
    cur = torch.tensor([0.0, 1.0, -0.0, 2.0, 0.5, -1.0])
    s = torch.full((6,), 7, dtype=torch.uint8)
    host.hostcheck_pass(_p(s), _p(cur), 6)
    assert s.tolist() == (cur != 0).to(torch.uint8).tolist() == [0, 1, 0, 1, 1, 1]
