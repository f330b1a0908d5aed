"""A real-valued (analog) Input on the HOST: the package's host path pinned to the reference-generated fixtures of
tests/golden/make_golden_analog.py (cases in tests/analog_cases.py).  The host path passes a float input through unchanged, as the
reference does (`Input.forward` is `self.s = x`, every compute() starts with `s.float()`); nothing pinned that until now.

Dyadic cases (every sum exact in f32): every field bit for bit.  Float cases: rasters, refrac_count and traces bit for bit, v and
summed within the spreads the generator measured against the stated order and stored.  The stated order itself (restated in numpy
in analog_cases.py) is held to the same fixtures, so that the GPU tests can pin the device to it bit for bit.  Then the 0/1
invariance: two existing byte fixtures of bindsnet.conversion, fed the same spikes as float32 zeros and ones."""
import numpy as np
import pytest
import torch

import analog_cases as AC
import conversion_cases as CC
import test_conversion_host as TCH


def _ns():
    from bindsnet_amd import conversion
    from bindsnet_amd.network import Network, nodes, topology
    from bindsnet_amd.network.monitors import Monitor
    ns = AC.ns_from(nodes, topology, Network, Monitor, conversion)
    ns.LIFNodes = nodes.LIFNodes
    return ns


@pytest.mark.parametrize("name", AC.CASES)
def test_host_path_equals_reference(name):
    g = AC.gold(name)
    ns = _ns()
    net = AC.build(ns, name, seed=int(g["seed"]))
    snaps = AC.run_case(ns, net, name)
    assert net.last_plan == "host-torch"
    AC.check_snapshots(name, snaps, g)


@pytest.mark.parametrize("name", AC.CASES)
def test_stated_order_equals_reference(name):
    """Half 2 of the float contract (and, for the dyadic family, that the stated order is exact too)."""
    g = AC.gold(name)
    if name not in AC.FLOAT:
        AC.assert_dyadic(name)
    snaps = AC.stated_run(name, seed=int(g["seed"]))
    AC.check_snapshots(name, snaps, g)
    if name in AC.FLOAT:
        margin = min(v for s in snaps for k, v in s.items() if k.endswith("_margin"))
        assert margin >= AC.MARGIN * float(g["v_spread"]), (margin, float(g["v_spread"]))
        assert margin == pytest.approx(float(g["least_margin"]), rel=1e-3)


def test_stated_products_on_zeros_and_ones_are_the_byte_order():
    """dense_real_stated / conv2d_real_stated on 0.0 / 1.0 values give the bits the byte order gives (the invariance, in numpy)."""
    rng = np.random.default_rng(5)
    s = (rng.random((3, 37)) < 0.4).astype(np.uint8)
    w, b = rng.standard_normal((37, 11)).astype(np.float32), rng.standard_normal(11).astype(np.float32)
    assert np.array_equal(AC.dense_real_stated(s.astype(np.float32), w, b).view(np.uint32), CC.dense_stated(s, w, b).view(np.uint32))
    s4 = (rng.random((2, 3, 7, 6)) < 0.4).astype(np.float32)
    w4, b4 = rng.standard_normal((5, 3, 3, 3)).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    torch.set_num_threads(1)
    want = torch.nn.functional.conv2d(torch.from_numpy(s4), torch.from_numpy(w4), torch.from_numpy(b4), padding=1).numpy()
    assert np.array_equal(AC.conv2d_real_stated(s4, w4, b4, pad=1).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", ["mlp_dy_b3", "cnn_dy"])
def test_zero_one_floats_give_the_byte_fixture(name, monkeypatch):
    """0/1 invariance on the host: an existing byte fixture of bindsnet.conversion, its spike trains fed as float32 0.0 / 1.0."""
    g = TCH.gold(name)
    ns = TCH._ns()
    byte_inputs = CC.case_inputs
    monkeypatch.setattr(CC, "case_inputs", lambda n, r: {k: v.float() for k, v in byte_inputs(n, r).items()})
    net = CC.build(ns, name, seed=int(g["seed"]))
    snaps = CC.run_case(ns, net, name)
    assert net.layers["Input"].s.dtype == torch.float32          # (the float slice went through as it was)
    TCH.check_snapshots(name, snaps, g)
