"""State monitors -- x, theta, refrac_count, i of layers and `activity` of MulticompartmentConnection(traces=True) -- on the HOST
path (plain PyTorch, network/host_path.py), pinned to the reference-generated fixtures of tests/golden/make_golden_state_monitors.py
(cases in tests/state_monitor_cases.py); the C entry point's argument checks, which need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import state_monitor_cases as SC


def ns():
    from bindsnet_amd.learning import MCC_learning
    from bindsnet_amd.network import Network, monitors, nodes, topology, topology_features
    return SC.ns_from(nodes, topology, topology_features, MCC_learning, Network, monitors)


def gold(name):
    return cases.gold("state_monitors_" + name)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.int64)


def check_snapshots(name, snaps):
    """Every record, final state tensor, feature value and the generator state against the fixture: bit for bit, except `activity`,
    which compares equal with zeros of either sign (the reference keeps -0.0 where a column's terms are all negative zeros)."""
    g = gold(name)
    for r, s in enumerate(snaps):
        for k, v in s.items():
            what = f"case {name} input {r}: {k}"
            want = g[f"r{r}_{k}"]
            if k.endswith("_s") and k.startswith(("rec_", "net_")):
                want = cases.unpack(want, tuple(g[f"r{r}_{k}_shape"]))
                assert v.shape == want.shape, f"{what}: shape {v.shape} vs {want.shape}"
                assert np.array_equal(v.astype(np.uint8), want), f"{what} differs ({int(v.sum())} vs {int(want.sum())} spikes)"
            elif k == "rng":
                assert np.array_equal(v, want), f"{what}: the run leaves the host generator elsewhere"
            elif k.startswith("act_"):
                assert v.shape == want.shape and v.dtype == want.dtype, f"{what}: {v.shape} {v.dtype} vs {want.shape} {want.dtype}"
                assert (want != 0).any(), f"{what}: vacuous"
                assert np.array_equal(v, want), f"{what} differs at {np.flatnonzero(v.reshape(-1) != want.reshape(-1))[:5]}"
            else:
                assert v.shape == want.shape and v.dtype == want.dtype, f"{what}: {v.shape} {v.dtype} vs {want.shape} {want.dtype}"
                got, ref = _bits(v).reshape(-1), _bits(want).reshape(-1)
                assert np.array_equal(got, ref), f"{what} differs at {np.flatnonzero(got != ref)[:5]}"
        stored = {k[len(f"r{r}_"):] for k in g.files if k.startswith(f"r{r}_") and not k.endswith("_shape")}
        assert stored == set(s), f"case {name} input {r}: fixture and run hold different records: {sorted(stored ^ set(s))}"


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_host_path_reproduces_reference_fixture(name):
    net = SC.build(ns(), name)
    snaps = SC.run_case(ns(), net, name)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps)


def test_traces_true_constructs_and_activity_has_the_reference_shape():
    n = ns()
    torch.manual_seed(0)
    X, Y = n.Input(n=6, traces=True), n.LIFNodes(n=5, traces=True)
    w = torch.rand(6, 5)
    conn = n.MulticompartmentConnection(X, Y, device="cpu", pipeline=[n.Weight("w", w.clone())], traces=True)
    assert conn.traces is True and conn.activity is None                 # topology.py:434-435
    s = (torch.rand(3, 6) < 0.5)
    out = conn.compute(s)
    assert tuple(conn.activity.shape) == (3, 5) and conn.activity.dtype == torch.float32
    assert tuple(out.shape) == (3, 5) and torch.equal(out, conn.activity)
    want = (w.unsqueeze(0) * s.view(3, 6, 1)).sum(1)
    assert torch.allclose(conn.activity, want, rtol=0, atol=1e-5)
    plain = n.MulticompartmentConnection(X, Y, device="cpu", pipeline=[n.Weight("w", w.clone())])
    assert plain.traces is False and not hasattr(plain, "activity")
    plain.compute(s)
    assert not hasattr(plain, "activity")


def test_record_entry_point_is_exported_and_checks_its_arguments_without_a_gpu():
    from bindsnet_amd import _lib
    L = _lib.lib()
    assert "snn_record_segments" in _lib.exported_symbols() and hasattr(L, "snn_record_segments")
    names = [f[0] for f in _lib.RunDesc._fields_]
    assert names[-2:] == ["records", "n_records"]
    assert [f[0] for f in _lib.RecordSegment._fields_] == ["src", "dst", "bytes"] and C.sizeof(_lib.RecordSegment) == 24
    assert [f[0] for f in _lib.ConnDesc._fields_][-1] == "activity"
    inv = _lib.lib().snn_error_string(-1)
    assert inv
    seg = (_lib.RecordSegment * 2)()
    # (addresses that are never dereferenced: every refusal below comes before anything is launched)
    seg[0].src, seg[0].dst, seg[0].bytes = 4096, 8192, 16
    seg[1].src, seg[1].dst, seg[1].bytes = 4096, 8192, 16
    assert L.snn_record_segments(seg, -1, 0, None) == -1, "negative n"
    assert L.snn_record_segments(seg, 2, -1, None) == -1, "negative t"
    assert L.snn_record_segments(None, 1, 0, None) == -1, "null table with n > 0"
    assert L.snn_record_segments(None, 0, 0, None) == 0, "nothing to do"
    seg[1].bytes = 18
    assert L.snn_record_segments(seg, 2, 0, None) == -1, "bytes not a multiple of 4"
    seg[1].bytes, seg[1].src = 16, None
    assert L.snn_record_segments(seg, 2, 0, None) == -1, "null source in a non-empty segment"
    seg[1].src, seg[1].dst = 4096, None
    assert L.snn_record_segments(seg, 2, 0, None) == -1, "null destination in a non-empty segment"
    seg[0].bytes = seg[1].bytes = 0
    seg[1].src = None
    assert L.snn_record_segments(seg, 2, 5, None) == 0, "empty segments are skipped, null pointers and all"


def test_a_run_refuses_a_bad_record_table_without_a_gpu():
    from bindsnet_amd import _lib
    L = _lib.lib()
    layers, R = (_lib.LayerDesc * 1)(), _lib.RunDesc()
    layers[0].kind, layers[0].n = _lib.LAYER_INPUT, 4
    layers[0].ext_spikes, layers[0].s = 4096, 4096
    R.B, R.T = 1, 1
    R.n_records = -1
    assert L.snn_net_run(layers, 1, None, 0, C.byref(R), None) == -1
    R.n_records, R.records = 1, None
    assert L.snn_net_run(layers, 1, None, 0, C.byref(R), None) == -1
    seg = (_lib.RecordSegment * 1)()
    seg[0].src, seg[0].dst, seg[0].bytes = 4096, 8192, 6
    R.records = seg
    assert L.snn_net_run(layers, 1, None, 0, C.byref(R), None) == -1
