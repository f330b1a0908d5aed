"""Per-neuron (tensor-valued) node parameters on the HOST path (plain PyTorch, network/host_path.py), pinned bit for bit to the
reference-generated fixtures of tests/golden/make_golden_pervec.py (cases in tests/pervec_cases.py); and the acceptance matrix the
generator stored: every class / parameter pair the reference runs constructs and runs here, every pair it refuses raises here."""
import numpy as np
import pytest
import torch

import cases
import pervec_cases as PC


def ns():
    from bindsnet_amd.learning import MCC_learning
    from bindsnet_amd.network import Network, nodes, topology, topology_features
    return PC.ns_from(nodes, topology, topology_features, MCC_learning, Network)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gold(name):
    return cases.gold("pervec_" + name)


def matrix():
    g = gold("matrix")
    return [str(p) for p in g["runs"]], [str(p) for p in g["raises"]]


def check_snapshots(name, snaps):
    """Every snapshot against the fixture: raster, every state tensor the layer has, the generator's state, Input trace, weights."""
    g = gold(name)
    for r, s in enumerate(snaps):
        want = cases.unpack(g[f"r{r}_raster"], s["raster"].shape)
        assert np.array_equal(s["raster"], want), f"case {name} input {r}: Y raster differs ({int(s['raster'].sum())} vs {int(want.sum())} spikes)"
        stored = sorted(k[len(f"r{r}_"):] for k in g.files if k.startswith(f"r{r}_") and k != f"r{r}_raster")
        assert stored == sorted(k for k in s if k != "raster"), f"case {name}: state tensors {sorted(s)} vs fixture {stored}"
        for k in stored:
            if k == "rng":
                assert np.array_equal(s[k], g[f"r{r}_rng"]), f"case {name} input {r}: the global generator is left elsewhere"
                continue
            got, ref = _bits(s[k]).reshape(-1), _bits(g[f"r{r}_{k}"]).reshape(-1)
            assert np.array_equal(got, ref), f"case {name} input {r}: {k} differs at {np.flatnonzero(got != ref)[:5]}"


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_fixture_meets_its_conditions(name):
    c, g = PC.CASES[name], gold(name)
    n = int(np.prod(c["shape"]))
    rasters = [cases.unpack(g[f"r{r}_raster"], (c["T"], c["B"], n)) for r in range(c["n_in"])]
    PC.conditions(name, rasters, [g[f"r{r}_theta"] for r in range(c["n_in"])] if "r0_theta" in g.files else None)
    yvec, xvec = PC.vectors(name)
    for v in list(yvec.values()) + list(xvec.values()):
        assert len(set(v.reshape(-1).tolist())) > n // 2, "a per-neuron parameter that hardly differs between neurons"


def test_matrix_is_the_table_of_the_reference():
    runs, raises = matrix()
    assert sorted(runs + raises) == sorted(PC.matrix_pairs())
    want = {"thresh", "tc_decay", "tc_i_decay", "tc_trace", "trace_scale+additive", "theta_plus", "tc_theta_decay"}
    assert {p.split(":")[1] for p in runs} == want
    assert {p.split(":")[1] for p in raises} == {"rest", "reset", "refrac", "lbound", "trace_scale"}
    assert "Input:tc_trace" in runs and "Input:trace_scale+additive" in runs


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_host_path_reproduces_reference_fixture(name):
    from bindsnet_amd.network.monitors import Monitor
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        net = PC.build(ns(), name)
        assert PC.sha(PC.weights(net).detach().numpy()) == str(gold(name)["w0_sha"])
        PC.load_derived(net, gold(name))
        snaps = PC.run_case(net, name, Monitor)
    finally:
        torch.set_num_threads(n)
    assert net.last_plan == "host-torch"
    check_snapshots(name, snaps)


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_compute_decays_makes_the_reference_buffers(name):
    """The derived per-neuron buffers are the reference's, bit for bit (the same torch.exp on the host).

    torch picks its vector exp by the CPU it runs on, and the last bit of single entries has been seen to differ between hosts
    (profiles/NOTES_pervec.md).  A failure here on a CPU other than the one the fixtures were made on, with every other test of
    this file green, says that about the host and nothing about compute_decays(): regenerate the fixtures on that host to check."""
    g = gold(name)
    mine = PC.derived(PC.build(ns(), name))
    assert sorted("derived_" + k for k in mine) == sorted(k for k in g.files if k.startswith("derived_"))
    for k, v in mine.items():
        assert np.array_equal(_bits(v), _bits(g["derived_" + k])), k


@pytest.mark.parametrize("pair", matrix()[0])
def test_host_path_runs_what_the_reference_runs(pair):
    out = PC.matrix_run(ns(), pair)
    assert len(out) == 4 and all(np.isfinite(v).all() for v, _, _, _ in out)


@pytest.mark.parametrize("pair", matrix()[1])
def test_host_path_refuses_what_the_reference_refuses(pair):
    with pytest.raises((RuntimeError, ValueError, TypeError, NotImplementedError)):
        PC.matrix_run(ns(), pair)


def test_parallel_modes_name_the_layer_and_the_parameter():
    from bindsnet_amd import parallel
    net = PC.build(ns(), "e_if")
    x = torch.from_numpy(PC.inputs("e_if", 0))
    for call in (lambda: parallel.sharded_run(net, {"X": x}, time=5), lambda: parallel.exact_run(net, {"X": x}, time=5),
                 lambda: parallel.column_shard(net, 0, 2)):
        with pytest.raises(NotImplementedError, match=r"'Y' \(IFNodes\).*`thresh`"):
            call()
