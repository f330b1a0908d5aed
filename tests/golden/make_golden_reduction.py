#!/usr/bin/env python3
"""Fixtures of the batch reductions mean / amax / amin of every learning rule: the UNMODIFIED reference's CPU path, one thread (build
container only), over the cases of tests/reduction_cases.py.  Writes tests/golden/reduction_<family>.npz: per case the run-level
record (per input the packed Y raster, W, the rule's state, rings and indices) and the update-level one (per connection.update() call
on set layer states: W and the rule's state).

The MCC cases are built with reduction=None and get `feature.learning_rule.reduction` assigned: the reference's
Weight(..., reduction=f) trips its own assertion for any f (topology_features.py:117-118, `isinstance(reduction, callable)`).

A fixture is written only if these hold on the reference's own output:
  * the output layer spikes in every input, and W moves (run-level and update-level);
  * W differs from the same base under torch.sum, and the three reductions differ from each other (batch > 1; at batch 1 all are
    equal): in the update calls, and for the dense and MCC graphs at the end of the runs too;
  * for amin at B = 3 some element's update is non-zero (W moves in an update-level call of every amin case at B = 3; at B = 33 only
    the reward rule's signed terms can give a non-zero minimum, and only there is it asked for);
  * for amax at B = 33 with MSTDP and a negative reward, some element's visited terms are all negative while a sample is skipped, so
    the result must be the zero the event-driven kernels fold in;
  * a clamp bound binds (run-level, on the weights before the normalisation, main shapes).

    python tests/golden/make_golden_reduction.py"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference/bindsnet"
for name, path in (("bindsnet", REF), ("bindsnet.analysis", REF + "/analysis")):
    pkg = types.ModuleType(name)
    pkg.__path__ = [path]
    sys.modules[name] = pkg
sys.modules["cv2"] = types.ModuleType("cv2")
import tv_shim  # noqa: E402
tv_shim.install()
import bindsnet.network  # noqa: E402,F401  (first, like the reference's own import order)
from bindsnet.learning import MCC_learning as ref_mcc, learning as ref_learning  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology, topology_features as ref_features  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import reduction_cases as RC  # noqa: E402

NS = RC.ns_from(ref_nodes, ref_topology, ref_features, ref_learning, ref_mcc, Network, Monitor)


def folded_zero_spy(found):
    """Before an update call of an MSTDP case: does some element have only negative non-zero terms reward * eligibility[b] and at
    least one sample whose term is zero?  Then amax must return that zero."""
    def spy(k, net):
        rule = RC.rule_of(net)
        elig = getattr(rule, "eligibility", None)
        if not isinstance(elig, torch.Tensor) or elig.dim() != 3:
            return
        t = RC.REWARDS[k % 2] * elig
        nz = t != 0
        hit = (nz.sum(0) > 0) & (nz.sum(0) < t.shape[0]) & (torch.where(nz, t, torch.full_like(t, -1.0)).amax(0) < 0)
        found.append(int(hit.sum()))
    return spy


def main():
    warnings.simplefilter("ignore")
    torch.set_num_threads(1)
    files = {}
    for base, c in RC.BASES.items():
        runs, ups = {}, {}
        for red in RC.REDUCTIONS:
            case = f"{base}_{red}" if red != "sum" else base
            found = []
            spy = folded_zero_spy(found) if (c["rule"], red, c["B"]) == ("MSTDP", "amax", 33) and not c.get("rvec") else None
            runs[red] = RC.run(NS, RC.build(NS, base, reduction=red), base)
            ups[red] = RC.run_updates(RC.build(NS, base, reduction=red), base, spy=spy)
            if spy is not None:
                assert sum(found) > 0, f"{case}: no element whose amax is the folded-in zero"
                print(case, "elements whose amax must be the folded-in zero, per call:", found)
        main_shape = c["shape"] == "main"
        for red in RC.TESTED:
            case = f"{base}_{red}"
            got, upd = runs[red], ups[red]
            # (amin keeps the depressing term wherever every sample has an event and little of the potentiating one: without a norm
            #  the layer may fall silent in the second input; so may the one weight of the smallest shape)
            assert (all if main_shape and red != "amin" else any)(g["raster"].sum() > 0 for g in got), f"{case}: the output layer does not spike"
            start = RC._np(RC.weights(RC.build(NS, base, reduction=red)))
            assert not np.array_equal(got[0]["w"], start), f"{case}: W does not move in the runs"
            moved = [not np.array_equal(a["w"], b) for a, b in zip(upd, [start] + [u["w"] for u in upd[:-1]])]
            # (amin over 33 samples at density 0.3 of terms that are never negative is zero wherever a sample is silent: there the
            #  case pins exactly that -- nothing but the clamp and the norm may move W)
            zero_update = red == "amin" and c["B"] == 33 and c["rule"] != "MSTDP"
            if not zero_update and (main_shape or red != "amin"):      # (a handful of weights: the minimum may be zero in all three calls)
                assert any(moved), f"{case}: W does not move in any update call"
            if c["B"] > 1 and main_shape:
                for other in RC.REDUCTIONS:
                    if other != red:
                        # (the convolutional graphs have no norm and are bistable -- all filters may end at a bound under more than
                        #  one reduction: there only the update-level calls below must differ)
                        differ = [not np.array_equal(g["w"], o["w"]) for g, o in zip(got, runs[other])]
                        assert differ[-1] or c["family"] not in ("dense", "mcc"), f"{case}: the runs end with the weights of {other}"
                        assert any(not np.array_equal(a["w"], b["w"]) for a, b in zip(upd, ups[other])), f"{case}: the updates equal {other}'s"
            elif c["B"] == 1:
                assert np.array_equal(got[-1]["w"], runs["sum"][-1]["w"]), f"{case}: batch 1 differs from torch.sum"
            # (WeightDependentPostPre scales its update by the distance to the bound: it approaches a bound and never lands on it)
            if main_shape and c["family"] in ("dense", "mcc") and not c.get("pv") and not zero_update and c["rule"] != "WeightDependentPostPre":
                pre = RC.run(NS, RC.build(NS, base, reduction=red, norm=False), base, n_in=1)[0]["w"]
                assert (pre == 0.0).any() or (pre == 1.0).any(), f"{case}: no clamp bound binds"
            files.setdefault(RC.fixture_of(case), {}).update(RC.pack(case, got, upd))
            print(case, [int(g["raster"].sum()) for g in got], "spikes; update calls that move W:", moved)
    for name, arrays in files.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        print(name, len(arrays), "arrays", os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20), name


if __name__ == "__main__":
    main()
