"""SparseConnection on the MI355X, bit for bit.

* Every fixture case of tests/golden/make_golden_sparse.py (tests/sparse_cases.py) through Network.run on the device, on the generic
  plan (the only plan such a graph takes), against the reference's recorded rasters and states.
* ops.prop_sparse (csrc/snn_sparse.hip) against ops.prop_dense on the densified matrix at the shapes of cases (c) and (g), with and
  without `accumulate` and a bias: both are the ascending-source order, so they must agree in every bit.  The limits the shapes
  straddle: 64 lanes per (256-column tile, sample) workgroup -- 37 columns (one partial tile), 700 (three tiles, the last partial);
  1024-source chunks -- 1100 and 2500 sources; a full row of 37 entries and segments of more than 64 entries (the dense block);
  batch 33 and 2.
* A changed `w` (edited in place, reassigned) is seen by the next compute() and the next run(); compute() on the device equals the
  host path's."""
import numpy as np
import pytest
import torch

import sparse_cases as SC
from test_sparse_host import _bits, _net, _ns, _pair, _some_w, check_snapshots

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_device_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    net = SC.build(_ns(), name).to(DEV)
    for conn in net.connections.values():
        assert conn.w.is_sparse and conn.w.is_cuda
    snaps = SC.run_case(net, name, Monitor, device=DEV)
    assert net.last_plan == "generic"
    check_snapshots(name, snaps)


def _shape_case(name, dense_block):
    """The case's first connection's matrix (optionally with a 40 x 200 block of stored entries: segments longer than a wave), and
    spikes at the case's batch size."""
    c = SC.CASES[name]
    spec = c["conns"][0]
    n_src, n_dst = c["inputs"][spec["src"]], c["n"]
    w, _ = SC.dense_weights(name, 0, n_src, n_dst)
    g = torch.Generator().manual_seed(c["seed"])
    if dense_block:
        w[1000:1040, :200] = torch.rand(40, min(200, n_dst), generator=g) - 0.5
    s = (torch.rand(c["B"], n_src, generator=g) < 0.2).to(torch.uint8)
    s[0, 1000:1040] = 1
    if c["B"] > 1:
        s[1] = 0                                              # a sample without a spike
    return w, s, torch.rand(n_dst, generator=g) - 0.5, torch.rand(c["B"], n_dst, generator=g)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("name,dense_block", [("c", False), ("g", False), ("g", True)])
def test_prop_sparse_equals_prop_dense_on_the_densified_matrix(name, dense_block, with_bias, accumulate):
    from bindsnet_amd import ops
    w, s, bias, prev = _shape_case(name, dense_block)
    wd, sd = w.to(DEV), s.to(DEV)
    bd = bias.to(DEV) if with_bias else None
    got, want = prev.to(DEV).clone(), prev.to(DEV).clone()
    ops.prop_sparse(ops.sparse_compile(wd.to_sparse()), sd, got, bias=bd, accumulate=accumulate)
    ops.prop_dense(wd.contiguous(), sd, want, bias=bd, accumulate=accumulate)
    torch.cuda.synchronize()
    got, want = got.cpu().numpy(), want.cpu().numpy()
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    assert bad.size == 0, f"{bad.size} of {got.size} sums differ from prop_dense (first {bad[:5]})"
    assert np.abs(want).sum() > 0
    # and both are the reference's own product (torch's sparse mm on the host)
    ref = s.float() @ w.to_sparse()
    if with_bias:
        ref = ref + bias
    ref = (prev + ref) if accumulate else ref
    assert np.array_equal(_bits(got), _bits(ref.numpy()))


def test_compute_on_the_device_equals_the_host_path():
    for name, k in (("b", 1), ("c", 0), ("g", 0)):
        host_net = SC.build(_ns(), name)
        conn_h = list(host_net.connections.values())[k]
        n_src = conn_h.source.n
        s = (torch.rand(5, n_src, generator=torch.Generator().manual_seed(k + n_src)) < 0.1).to(torch.uint8)
        want = conn_h.compute(s)
        conn_d = list(SC.build(_ns(), name).to(DEV).connections.values())[k]
        got = conn_d.compute(s.to(DEV))
        assert got.is_cuda and got.shape == want.shape
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want.numpy())), name


def test_changed_weights_are_seen_by_the_next_compute_on_the_device():
    w = _some_w()
    c = _pair(w=w).to(DEV)
    s = torch.ones(1, 12, dtype=torch.uint8)
    sd = s.to(DEV)
    assert c.w.is_sparse and c.w.is_cuda
    first = c.compute(sd).cpu()
    assert torch.equal(first, s.float() @ w)
    ptr0 = c.sp_val.data_ptr()
    assert torch.equal(c.compute(sd).cpu(), first) and c.sp_val.data_ptr() == ptr0, "an unchanged w is compiled once"
    c.w *= 2                                                   # in place (the values move, the Parameter stays)
    assert torch.equal(c.compute(sd).cpu(), s.float() @ (w * 2))
    c.w._values().mul_(0.5)                                    # in place on the values alone
    assert torch.equal(c.compute(sd).cpu(), first)
    w2 = _some_w(seed=9)
    c.w = torch.nn.Parameter(w2.to_sparse().to(DEV), requires_grad=False)
    assert torch.equal(c.compute(sd).cpu(), s.float() @ w2)


def test_changed_weights_are_seen_by_the_next_run_on_the_device():
    """Three runs of the same input from the same state: the kept run descriptors must not outlive an in-place edit of the values
    (nothing is assigned, no address moves) nor a reassignment; each run equals a fresh host network with those weights."""
    w = 0.02 * (_some_w() + 0.5)
    x = torch.ones(20, 1, 12, dtype=torch.uint8)

    def host_v(weights):
        net = _net(_pair(w=weights))
        net.run({"X": x.clone()}, time=20)
        return net.layers["Y"].v.clone()

    net = _net(_pair(w=w)).to(DEV)
    conn = net.connections[("X", "Y")]
    xd = x.to(DEV)
    seen = []
    for edit in (lambda: None, lambda: conn.w._values().mul_(2.0),
                 lambda: setattr(conn, "w", torch.nn.Parameter((3.0 * w).to_sparse().to(DEV), requires_grad=False))):
        edit()
        net.run({"X": xd.clone()}, time=20)
        assert net.last_plan == "generic"
        seen.append(net.layers["Y"].v.cpu().clone())
        net.reset_state_variables()
    for got, factor in zip(seen, (1.0, 2.0, 3.0)):
        assert np.array_equal(_bits(got.numpy()), _bits(host_v(factor * w).numpy())), factor
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_refusals_on_the_device_leave_the_state_alone():
    w = _some_w() + 5.0
    x = {"X": torch.ones(3, 1, 12, dtype=torch.uint8, device=DEV)}
    for make, exc, wording, kwargs in (
            (lambda: _net(_pair(w=w, norm=1.0)), NotImplementedError, r"normalize\(\) raises", {}),
            (lambda: _net(_pair(w=w)), Exception, r"^Mask isn't supported for SparseConnection$",
             {"masks": {("X", "Y"): torch.zeros(12, 7, dtype=torch.bool)}}),
            (lambda: _net(_pair(w=w), monitor_w=True), NotImplementedError, "monitor", {})):
        net = make().to(DEV)
        net.layers["Y"].set_batch_size(1)
        v0 = net.layers["Y"].v.clone()
        with pytest.raises(exc, match=wording):
            net.run(dict(x), time=3, **kwargs)
        assert torch.equal(net.layers["Y"].v, v0)
