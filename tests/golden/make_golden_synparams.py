#!/usr/bin/env python3
"""Fixtures of per-synapse learning rates, weight bounds and per-target norms: the UNMODIFIED reference's CPU path (build container
only) over the cases of tests/synparams_cases.py.  Writes tests/golden/synparams_op_<rule>.npz (the op-level cases of one rule),
synparams_run.npz (the run-level cases) and synparams_raises.json (exception type and message of every cell that fails).

A fixture is written only if, for every case, the conditions of synparams_cases.op_conditions / run_conditions hold on the
reference's own output: output spikes, w moves, each tensor bound binds on elements whose bound values differ, the result differs
from the run with every tensor replaced by its mean, and a column's norm / colsum differs from norm * (1 / colsum).

    python tests/golden/make_golden_synparams.py"""
import json
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
from bindsnet.learning import learning as ref_learning, MCC_learning as ref_mcc  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology, topology_features as ref_features  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import synparams_cases as SC  # noqa: E402

NS = SC.ns_from(ref_nodes, ref_topology, ref_features, ref_learning, ref_mcc, Network, Monitor)


def main():
    warnings.simplefilter("ignore")
    torch.set_num_threads(1)
    by_rule = {}
    for case, c in SC.OP_CASES.items():
        got = SC.run_op(*SC.build_op(NS, case), case)
        mean = SC.run_op(*SC.build_op(NS, case, "mean"), case)
        SC.op_conditions(case, got, mean)
        for key, a in got.items():
            by_rule.setdefault(c["rule"], {})[f"{case}/{key}"] = a
    for rule, arrays in by_rule.items():
        np.savez_compressed(os.path.join(HERE, f"synparams_op_{rule}.npz"), **arrays)
        print(rule, len(arrays), "arrays")
    arrays = {}
    for case in SC.RUN_CASES:
        got = SC.run_run(NS, SC.build_run(NS, case), case)
        mean = SC.run_run(NS, SC.build_run(NS, case, "mean"), case)
        SC.run_conditions(case, got, mean, *SC.pre_norm_weights(NS, case))
        for r, g in enumerate(got):
            arrays[f"{case}/raster{r}"] = np.packbits(g["raster"])
            arrays[f"{case}/w{r}"] = g["w"]
            arrays[f"{case}/v{r}"] = g["v"]
        print(case, [int(g["raster"].sum()) for g in got], "spikes")
    np.savez_compressed(os.path.join(HERE, "synparams_run.npz"), **arrays)
    raises = {}
    for name in SC.RAISES:
        try:
            SC.raises_trial(NS, name)
            raises[name] = {"type": "ok", "message": ""}
        except Exception as e:      # noqa: BLE001
            raises[name] = {"type": type(e).__name__, "message": str(e).splitlines()[0][:200]}
        print(name, raises[name]["type"])
    assert all(v["type"] != "ok" for v in raises.values()), raises
    with open(os.path.join(HERE, "synparams_raises.json"), "w") as f:
        json.dump(raises, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
