#!/usr/bin/env python3
"""Fixtures of Weight(norm_frequency="time step"): the UNMODIFIED reference's CPU path, one thread (build container only), over the
cases of tests/norm_step_cases.py.  Writes tests/golden/norm_step_<case>.npz: per input the packed rasters, every layer's v, theta,
refrac_count and trace, every feature value, the rule state of every Weight (p_plus, p_minus, eligibility_trace, rings, ring indices)
and the global generator's state.

A fixture is written only if norm_step_cases.conditions holds on the reference's own output: every input makes every layer spike,
the rasters of (a) differ from the same case with norm_frequency="sample", the learned weights differ from that mode's, and fewer
than 25 % of the final weights lie at a bound.  For (c), NoOp with train(False), the column sums are checked to equal the norm.

    python tests/golden/make_golden_norm_step.py"""
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
from bindsnet.learning import MCC_learning as ref_mcc  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology, topology_features as ref_features  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import norm_step_cases as NC  # noqa: E402

NS = NC.ns_from(ref_nodes, ref_topology, ref_features, ref_mcc, Network, Monitor)


def run(case, frequency):
    torch.manual_seed(NC.CASES[case]["seed"])
    return NC.run(NS, NC.build(NS, case, frequency=frequency), case)


def main():
    warnings.simplefilter("ignore")
    torch.set_num_threads(1)
    for case, c in NC.CASES.items():
        got, sample = run(case, "time step"), run(case, "sample")
        NC.conditions(case, got, sample)
        if case == "c":
            for g in got:
                sums = g["feat_X_Y_0"].astype(np.float64).sum(0)
                assert np.allclose(sums, c["norm"], rtol=1e-5), sums
        path = os.path.join(HERE, f"norm_step_{case}.npz")
        np.savez_compressed(path, **NC.pack(case, got))
        print(case, [{k: int(v.sum()) for k, v in g.items() if k.startswith("raster_")} for g in got], f"{100 * NC.at_bound(case, got):.1f} % at a bound,",
              os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
