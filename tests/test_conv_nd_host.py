"""Conv1dConnection / Conv3dConnection with PostPre on the HOST: the package's host path (plain PyTorch, network/host_path.py)
pinned bit for bit to the reference-generated fixtures of tests/golden/make_golden_conv_nd.py (cases in tests/conv_nd_cases.py);
the PostPre gather table against the reference's unfold; the order-carrying bodies of bindsnet_amd/csrc/snn_convnd.hpp, compiled
for the CPU (tests/hostcheck/convnd_host.hip), against F.conv1d / F.conv3d and the reference's bmm bodies; the unsupported
options."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
import conv_nd_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _ns():
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network, nodes, topology
    return CC.ns_from(nodes, topology, learning, Network)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_snapshots(name, snaps, first=0, w_atol=None):
    """Every recorded quantity bit for bit (w within w_atol when given, the raster still exact)."""
    g = cases.gold("convnd_" + name)
    c = CC.CASES[name]
    for i, s in enumerate(snaps):
        r = first + i
        want = cases.unpack(g[f"r{r}_raster"], s["raster"].shape)
        assert np.array_equal(s["raster"], want), f"case {name} input {r}: Y raster differs ({int(s['raster'].sum())} vs {int(want.sum())} spikes)"
        for k in ("v", "refrac", "theta", "xY", "gen"):
            got, ref = _bits(s[k]).reshape(-1), _bits(g[f"r{r}_{k}"]).reshape(-1)
            assert np.array_equal(got, ref), f"case {name} input {r}: {k} differs at {np.flatnonzero(got != ref)[:5]}"
        if f"r{r}_xX" in g.files:
            assert np.array_equal(_bits(s["xX"]).reshape(-1), _bits(g[f"r{r}_xX"]).reshape(-1)), f"case {name} input {r}: xX differs"
        else:
            assert CC.sha(s["xX"]) == str(g[f"r{r}_xX_sha"]), f"case {name} input {r}: xX differs"
        ref_w = g[f"r{r}_w"] if f"r{r}_w" in g.files else (g["final_w"] if r == c["n_in"] - 1 and "final_w" in g.files else None)
        if w_atol is not None:
            if ref_w is not None:
                np.testing.assert_allclose(s["w"], ref_w, rtol=0, atol=w_atol)
            continue
        if ref_w is not None:
            got, ref = _bits(s["w"]).reshape(-1), _bits(ref_w).reshape(-1)
            assert np.array_equal(got, ref), f"case {name} input {r}: w differs at {np.flatnonzero(got != ref)[:5]}"
        assert CC.sha(s["w"]) == str(g[f"r{r}_w_sha"]), f"case {name} input {r}: w differs"


def test_classes_mirror_the_reference_hierarchy():
    from bindsnet.network import topology
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input
    from bindsnet_amd.network.topology import AbstractConnection, Conv2dConnection
    assert issubclass(topology.Conv1dConnection, AbstractConnection) and issubclass(topology.Conv3dConnection, AbstractConnection)
    assert not issubclass(topology.Conv1dConnection, Conv2dConnection) and not issubclass(topology.Conv3dConnection, Conv2dConnection)
    X, Y = Input(shape=[2, 20]), DiehlAndCookNodes(shape=[3, 10])
    c = topology.Conv1dConnection(X, Y, kernel_size=4, stride=2, padding=1)
    assert tuple(c.w.shape) == (3, 2, 4) and torch.equal(c.b, torch.zeros(3))
    assert (c.kernel_size, c.stride, c.padding, c.dilation) == (4, 2, 1, 1)
    X3, Y3 = Input(shape=[1, 6, 6, 6]), DiehlAndCookNodes(shape=[2, 3, 3, 3])
    c3 = topology.Conv3dConnection(X3, Y3, kernel_size=3, stride=2, padding=1)
    assert tuple(c3.w.shape) == (2, 1, 3, 3, 3) and c3.kernel_size == (3, 3, 3) and c3.padding == (1, 1, 1)
    Y.set_batch_size(1)
    Y.v.fill_(-50.0)
    c.reset_state_variables()                         # unlike the Local classes, the target is left alone
    assert float(Y.v.view(-1)[0]) == -50.0


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_construction_draws_the_fixture_weights(name):
    net = CC.build(_ns(), name)
    assert CC.sha(CC.conn_of(net).w.detach().numpy()) == str(cases.gold("convnd_" + name)["w0_sha"])


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_host_path_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        net = CC.build(_ns(), name)
        snaps = CC.run_case(net, name, Monitor)
    finally:
        torch.set_num_threads(n)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps)


def _ref_pp_matrix_1d(Cin, N, K, s, p):
    """learning.py:434-438 written out on arange: flat source index + 1, 0 for padding."""
    t = F.pad((torch.arange(Cin * N) + 1).view(1, Cin, N).float(), (p, p))
    return t.unfold(-1, K, s).reshape(1, -1, Cin * K)[0].long() - 1


@pytest.mark.parametrize("Cin,N,K,s,p", [(1, 784, 56, 28, 0), (2, 60, 6, 2, 1), (3, 17, 4, 3, 2), (16, 9, 3, 1, 1)])
def test_pp_table_1d_is_the_reference_unfold(Cin, N, K, s, p):
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input
    from bindsnet_amd.network.topology import Conv1dConnection
    L = (N - K + 2 * p) // s + 1
    c = Conv1dConnection(Input(shape=[Cin, N]), DiehlAndCookNodes(shape=[2, L]), kernel_size=K, stride=s, padding=p)
    assert c.pp_src.dtype == torch.int32 and tuple(c.pp_src.shape) == (L, Cin * K)
    assert torch.equal(c.pp_src.long(), _ref_pp_matrix_1d(Cin, N, K, s, p))
    if Cin > 1:        # the raw reshape: row l is NOT the channels of window l
        assert not torch.equal(c.pp_src[1].long(), torch.tensor([ci * N + 1 * s - p + k for ci in range(Cin) for k in range(K)]))


@pytest.mark.parametrize("shape,k,s,p", [((6, 6, 6), 3, 2, 1), ((28, 28, 28), 16, 4, 0), ((5, 7, 6), (3, 3, 2), 1, 0)])
def test_pp_table_3d_is_the_reference_unfold(shape, k, s, p):
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input
    from bindsnet_amd.network.topology import Conv3dConnection
    ks = k if isinstance(k, tuple) else (k,) * 3
    out = [(n - kk + 2 * p) // s + 1 for n, kk in zip(shape, ks)]
    c = Conv3dConnection(Input(shape=[1, *shape]), DiehlAndCookNodes(shape=[2, *out]), kernel_size=k, stride=s, padding=p)
    t = F.pad((torch.arange(int(np.prod(shape))) + 1).view(1, 1, *shape).float(), (p,) * 6)
    try:           # learning.py:523-534: D unfolded with the kernel's width, W with its depth
        ref = t.unfold(-3, ks[2], s).unfold(-3, ks[1], s).unfold(-3, ks[0], s).reshape(1, -1, ks[0] * ks[1] * ks[2])[0].long() - 1
    except RuntimeError:
        ref = None
    if ref is not None and ref.shape[0] == int(np.prod(out)):
        assert c._pp_error is None and torch.equal(c.pp_src.long(), ref)
    else:
        assert c._pp_error is not None and c.pp_src.shape[0] == 0


# ---- the host-compiled bodies of snn_convnd.hpp --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libconvndhost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "convnd_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    lib.hostcheck_convnd_prop.argtypes = [C.c_void_p] * 3 + [C.c_int] * 11 + [C.c_void_p]
    lib.hostcheck_convnd_pp.argtypes = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p] * 2
    return lib


def _p(t):
    return C.c_void_p(t.data_ptr())


PROP_SWEEP = [  # Cin, spatial, kernel, stride, pad, Cout, B, density
    (1, (784,), 56, 28, 0, 25, 1, 0.05), (1, (784,), 56, 28, 2, 5, 3, 0.3), (2, (60,), 6, 2, 1, 4, 3, 0.2),
    (4, (33,), 5, 1, 2, 3, 2, 0.4), (16, (40,), 7, 3, 1, 3, 2, 0.3), (16, (12,), 1, 1, 0, 2, 1, 0.5),
    (1, (28, 28, 28), 16, 4, 0, 3, 1, 0.03), (1, (9, 10, 11), 4, 2, 0, 3, 1, 0.3), (1, (6, 6, 6), 3, 2, 1, 2, 2, 0.5),
    (1, (8, 8, 8), (3, 2, 4), 1, 2, 2, 1, 0.3), (1, (40, 3, 3), 3, 1, 0, 2, 1, 1.0),
]


@pytest.mark.parametrize("case", PROP_SWEEP)
def test_chain_body_equals_torch_conv(host, case):
    Cin, spatial, k, s, p, Cout, B, d = case
    torch.manual_seed(sum(spatial) + Cin)
    ks = (k,) * len(spatial) if not isinstance(k, tuple) else k
    W = torch.rand(Cout, Cin, *ks) - 0.3
    bias = torch.rand(Cout) - 0.5
    spk = (torch.rand(B, Cin, *spatial) < d).to(torch.uint8)
    conv = F.conv1d if len(spatial) == 1 else F.conv3d
    for b in (None, bias):
        want = conv(spk.float(), W, b, stride=s, padding=p).contiguous()
        got = torch.full_like(want, float("nan"))
        dims = (1, 1, *spatial) if len(spatial) == 1 else spatial
        kd = (1, 1, *ks) if len(spatial) == 1 else ks
        assert host.hostcheck_convnd_prop(_p(W), None if b is None else _p(b), _p(spk), B, Cin, *dims, Cout, *kd, s, p, _p(got)) == 0
        assert np.array_equal(_bits(got.numpy()), _bits(want.numpy())), f"chain differs at {np.flatnonzero(_bits(got.numpy()) != _bits(want.numpy()))[:5]}"


PP_SWEEP = [  # kind, Cin, spatial, k, s, p, Cout, B, density of the target spikes
    ("c1", 1, (784,), 56, 28, 0, 25, 1, 0.05), ("c1", 2, (60,), 6, 2, 1, 4, 3, 0.2), ("c1", 3, (17,), 4, 3, 2, 2, 2, 0.5),
    ("c1", 16, (20,), 3, 1, 1, 2, 2, 1.0), ("c3", 1, (28, 28, 28), 16, 4, 0, 2, 1, 0.05), ("c3", 1, (6, 6, 6), 3, 2, 1, 3, 2, 0.3),
    ("c1", 1, (100,), 1, 1, 0, 2, 2, 0.3),
]


@pytest.mark.parametrize("case", PP_SWEEP)
def test_postpre_bodies_equal_reference_bmm(host, case):
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input
    from bindsnet_amd.network.topology import Conv1dConnection, Conv3dConnection
    kind, Cin, spatial, k, s, p, Cout, B, d = case
    out = [(n - k + 2 * p) // s + 1 for n in spatial]
    cls = Conv1dConnection if kind == "c1" else Conv3dConnection
    c = cls(Input(shape=[Cin, *spatial]), DiehlAndCookNodes(shape=[Cout, *out]), kernel_size=k, stride=s, padding=p)
    g = torch.Generator().manual_seed(Cout * 7 + B)
    n_src, L, J = Cin * int(np.prod(spatial)), int(np.prod(out)), c.pp_src.shape[1]
    s_src = (torch.rand(B, n_src, generator=g) < 0.3).to(torch.uint8)
    x_src = torch.rand(B, n_src, generator=g) * (torch.rand(B, n_src, generator=g) < 0.6)
    s_tgt = (torch.rand(B, Cout, L, generator=g) < d).to(torch.uint8)
    x_tgt = torch.rand(B, Cout, L, generator=g) * (torch.rand(B, Cout, L, generator=g) < 0.6)
    pre, post = torch.full((B, Cout, J), float("nan")), torch.full((B, Cout, J), float("nan"))
    tab = c.pp_src.contiguous()
    assert host.hostcheck_convnd_pp(_p(tab), _p(s_src), _p(x_src), _p(s_tgt), _p(x_tgt), B, Cout, L, J, n_src, _p(pre), _p(post)) == 0
    shape = (B, Cin, *spatial)
    want_pre = torch.bmm(x_tgt, c._pp_unfold(s_src.view(shape).float()))
    want_post = torch.bmm(s_tgt.float(), c._pp_unfold(x_src.view(shape)))
    assert np.array_equal(_bits(pre.numpy()), _bits(want_pre.numpy()))
    assert np.array_equal(_bits(post.numpy()), _bits(want_post.numpy()))


# ---- what is not supported ---------------------------------------------------------------------------------------------
def test_unsupported_options_raise():
    from bindsnet_amd import parallel
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input
    from bindsnet_amd.network.topology import Conv1dConnection, Conv3dConnection
    X1, Y1 = Input(shape=[1, 20], traces=True), DiehlAndCookNodes(shape=[2, 9], traces=True)
    X3, Y3 = Input(shape=[1, 6, 6, 6], traces=True), DiehlAndCookNodes(shape=[2, 3, 3, 3], traces=True)
    with pytest.raises(NotImplementedError, match="Dilation"):
        Conv1dConnection(X1, Y1, kernel_size=4, stride=2, dilation=2)
    with pytest.raises(NotImplementedError, match="Dilation"):
        Conv3dConnection(X3, Y3, kernel_size=3, stride=2, padding=1, dilation=2)
    with pytest.raises(AssertionError):
        Conv1dConnection(X1, Y1, kernel_size=4, stride=3)
    with pytest.raises(NotImplementedError, match="16 input channels"):
        Conv1dConnection(Input(shape=[17, 20]), Y1, kernel_size=4, stride=2)
    with pytest.raises(NotImplementedError, match="one input channel"):
        Conv3dConnection(Input(shape=[2, 6, 6, 6]), Y3, kernel_size=3, stride=2, padding=1)
    with pytest.raises(NotImplementedError, match="isotropic"):
        Conv3dConnection(Input(shape=[1, 6, 6, 7]), DiehlAndCookNodes(shape=[2, 3, 3, 3]), kernel_size=3, stride=(2, 2, 2),
                         padding=(1, 1, 0))
    for rule in (learning.Hebbian, learning.WeightDependentPostPre, learning.MSTDP, learning.MSTDPET):
        with pytest.raises(NotImplementedError):
            Conv1dConnection(X1, Y1, kernel_size=4, stride=2, nu=0.1, update_rule=rule, wmin=0.0, wmax=1.0)
    # conv3d PostPre with nu[0] != 0: the reference's bmm fails; here run() raises before any state changes
    c3 = Conv3dConnection(X3, Y3, kernel_size=3, stride=2, padding=1, update_rule=learning.PostPre, nu=(1e-2, 1e-2), wmax=1.0)
    net = Network()
    net.add_layer(X3, "X"); net.add_layer(Y3, "Y"); net.add_connection(c3, "X", "Y")
    w0, v0, th0, rng0 = c3.w.clone(), Y3.v.clone(), Y3.theta.clone(), torch.get_rng_state()
    x = torch.ones(4, 1, 1, 6, 6, 6, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="float != bool"):
        net.run({"X": x}, time=4)
    assert torch.equal(c3.w, w0) and torch.equal(Y3.v, v0) and torch.equal(Y3.theta, th0)
    assert torch.equal(torch.get_rng_state(), rng0) and float(X3.x.abs().sum()) == 0.0
    net.train(False)
    net.run({"X": x}, time=4)                            # learning off: the rule is never called
    net.train(True)
    c3.update_rule.nu[0] = 0.0
    net.run({"X": x}, time=4)                            # nu[0] == 0: the post term only
    # masks and the multi-device modes
    c1 = Conv1dConnection(X1, Y1, kernel_size=4, stride=2, update_rule=learning.PostPre, nu=(1e-2, 1e-2), wmax=1.0)
    net1 = Network()
    net1.add_layer(X1, "X"); net1.add_layer(Y1, "Y"); net1.add_connection(c1, "X", "Y")
    with pytest.raises(NotImplementedError, match="masks"):
        net1.run({"X": torch.zeros(2, 1, 1, 20, dtype=torch.uint8)}, time=2, masks={("X", "Y"): torch.zeros(2, 1, 4, dtype=torch.bool)})
    with pytest.raises(NotImplementedError, match="Conv1dConnection"):
        parallel.column_shard(net1, 0, 2)
    with pytest.raises(NotImplementedError, match="Conv1dConnection"):
        parallel.sharded_run(net1, {"X": torch.zeros(2, 1, 1, 20, dtype=torch.uint8)}, time=2)
    with pytest.raises(NotImplementedError, match="Conv3dConnection"):
        parallel._exact_check(net)
