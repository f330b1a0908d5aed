"""Weight(norm_frequency="time step") on the device (include/snnhip.h f16: snn_prop_cascade_norm_f32 / snn_prop_cascade_norm_pv_f32, and
the generic plan of snn_net_run, which normalises such a Weight behind its propagation in every timestep):

  * the fused entry points against the two-call sequence snn_prop_cascade_f32 + snn_normalize(_pv), bit for bit in `out` and in W:
    the shapes of the host check, one column, the 4..7 column class, more samples than one pass, and a matrix whose tile does not fit
    the LDS (the entry point's own fall-back); densities 0, 5 % and 100 %; accumulate 0 and 1; a scalar and a per-target norm;
    negative weights, an all-zero column and a column that sums to exactly 0;
  * every fixture case of tests/norm_step_cases.py (written by the unmodified reference) through Network.run, bit for bit, on the
    generic plan -- in both forms the plan has for a single Weight (the two calls, the fused launch);
  * compute() by hand normalises as a step of run() does; normalize() is a no-op;
  * a kept run descriptor notices norm_frequency being reassigned between runs."""
import numpy as np
import pytest
import torch

import norm_step_cases as NC
from test_norm_step_host import HERE, ns, run_fixture
from test_norm_step_hostcheck import EXTRA, SHAPES, operands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BEYOND_LDS = ((1300, 20, 2),)       # 1300 rows x 16 columns with their spike lists: more than a workgroup's LDS


@pytest.mark.parametrize("shape", SHAPES + EXTRA + BEYOND_LDS)
@pytest.mark.parametrize("vector", (False, True))
def test_fused_entry_equals_the_two_calls(shape, vector):
    from bindsnet_amd import ops
    Nin, N, B = shape
    norm = torch.linspace(0.5, 2.5, N, device=DEV) if vector else 0.1 * Nin
    for density in (0.0, 0.05, 1.0):
        for accumulate in (False, True):
            W, s, out0 = (t.to(DEV) for t in operands(Nin, N, B, density, 1000 * Nin + N + int(100 * density)))
            want_W, want_out = W.clone(), out0.clone()
            ops.prop_cascade(want_W, s, want_out, accumulate=accumulate)
            ops.normalize(want_W, norm, use_abs=False)
            got_W, got_out = W.clone(), out0.clone()
            ops.prop_cascade_norm(got_W, s, got_out, norm, accumulate=accumulate)
            assert torch.equal(got_out, want_out), (shape, density, accumulate, int((got_out != want_out).sum()))
            assert torch.equal(got_W, want_W), (shape, density, accumulate, int((got_W != want_W).sum()))


@pytest.mark.parametrize("form", (1, 2), ids=("two_calls", "fused"))
@pytest.mark.parametrize("case", sorted(NC.CASES))
def test_fixture_case_bit_for_bit_on_the_generic_plan(case, form, monkeypatch):
    from bindsnet_amd.network.topology import MulticompartmentConnection
    monkeypatch.setattr(MulticompartmentConnection, "_NORM_STEP_FORM", form)
    net, got = run_fixture(ns(), case, device=DEV)
    assert net.last_plan == "generic"
    NC.assert_same(case, got, NC.gold(case, HERE), f"device, form {form}")


@pytest.mark.parametrize("form", (1, 2), ids=("two_calls", "fused"))
def test_compute_by_hand_normalises_and_normalize_does_not(form, monkeypatch):
    from bindsnet_amd.network.topology import MulticompartmentConnection
    monkeypatch.setattr(MulticompartmentConnection, "_NORM_STEP_FORM", form)
    NS = ns()
    net = NC.build(NS, "c")
    net.to(DEV)
    conn = net.connections[("X", "Y")]
    feat = NC.weights(net)["X_Y"]
    before = feat.value.detach().clone()
    feat.normalize()
    conn.normalize()
    assert torch.equal(feat.value, before)
    s = torch.from_numpy(NC.inputs("c", 0)["X"][0]).to(DEV)
    out = conn.compute(s)
    want = torch.empty_like(out)
    from bindsnet_amd import ops
    ops.prop_cascade(before, s, want)
    assert torch.equal(out, want)
    ops.normalize(before, 4.0, use_abs=False)
    assert torch.equal(feat.value, before)


def test_kept_descriptor_notices_a_reassigned_frequency():
    NS = ns()
    net = NC.build(NS, "a")
    net.to(DEV)
    feat = NC.weights(net)["X_Y"]
    x = [torch.from_numpy(NC.inputs("a", r)["X"]).to(DEV) for r in range(2)]
    sums = lambda: feat.value.detach().double().sum(0).cpu().numpy()      # noqa: E731
    torch.manual_seed(1)
    net.run({"X": x[0]}, time=30)
    net.run({"X": x[0]}, time=30)                       # (the second plain call runs from the kept descriptors)
    assert not np.allclose(sums(), 4.0, rtol=1e-5)      # the last update follows the last normalisation
    feat.norm_frequency = "sample"
    net.run({"X": x[1]}, time=30)
    assert np.allclose(sums(), 4.0, rtol=1e-5)          # the run's closing normalisation is back
    feat.norm_frequency = "time step"
    net.run({"X": x[1]}, time=30)
    assert not np.allclose(sums(), 4.0, rtol=1e-5)
    assert net.last_plan == "generic"
