#!/usr/bin/env python3
"""Fixtures of the per-neuron (tensor-valued) node parameters: the UNMODIFIED reference's CPU path (build container only) over
the cases of tests/pervec_cases.py.  Per input: the Y raster (bit-packed), v, refrac_count, x and theta / i / u where the class
has them, the global generator's state for the one_spike cases, and w plus the Input trace for the PostPre case.

It first re-runs the acceptance matrix (pervec_cases.MATRIX: every class x parameter, one [n] tensor at a time, B = 1 and 3, two
runs with reset_state_variables() between them) and stores which pairs the reference runs and which it refuses as
pervec_matrix.npz -- the contract of the host path and of the device path.  Case (f) and the Input rows of the contract stand on
`Input:tc_trace` and `Input:trace_scale+additive` running there; the generator stops if they do not.

    python tests/golden/make_golden_pervec.py"""
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
from bindsnet.learning import MCC_learning as ref_mcc_learning  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology, topology_features as ref_features  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import pervec_cases as PC  # noqa: E402
from dt_cases import save_fixture  # noqa: E402


def matrix(ns):
    runs, raises = [], []
    for pair in PC.matrix_pairs():
        try:
            PC.matrix_run(ns, pair)
            runs.append(pair)
        except Exception as e:                      # whatever torch or the reference raises: the pair is refused
            raises.append(pair)
            print(f"  {pair}: {type(e).__name__}: {str(e).splitlines()[0][:90]}")
    return runs, raises


def main():
    torch.set_num_threads(1)
    warnings.filterwarnings("ignore", category=UserWarning)        # (torch.tensor(tensor) in the reference's constructors)
    ns = PC.ns_from(ref_nodes, ref_topology, ref_features, ref_mcc_learning, Network)
    runs, raises = matrix(ns)
    print("the reference runs", len(runs), "pairs and refuses", len(raises))
    assert "Input:tc_trace" in runs and "Input:trace_scale+additive" in runs, "case (f) needs per-neuron traces on Input layers"
    np.savez_compressed(os.path.join(HERE, "pervec_matrix.npz"), runs=np.array(runs), raises=np.array(raises))
    for name in PC.CASES:
        net = PC.build(ns, name)
        w0 = PC.weights(net).detach().numpy().copy()
        snaps = PC.run_case(net, name, Monitor)
        PC.conditions(name, [s["raster"] for s in snaps], [s["theta"] for s in snaps] if "theta" in snaps[0] else None)
        out = {"w0_sha": np.array(PC.sha(w0)), "seed": np.array(PC.CASES[name]["seed"])}
        out.update({"derived_" + k: v for k, v in PC.derived(net).items()})
        for r, s in enumerate(snaps):
            out[f"r{r}_raster"] = np.packbits(s["raster"].reshape(-1))
            for k, v in s.items():
                if k != "raster":
                    out[f"r{r}_{k}"] = v
        path = os.path.join(HERE, f"pervec_{name}.npz")
        c = PC.CASES[name]
        if "dt" in c:           # (McCullochPitts and IzhikevichNodes have no refractory period)
            save_fixture(path, out, name, [s["raster"] for s in snaps], os.path.join(HERE, f"pervec_{c['sibling']}.npz"),
                         refractory=c["kind"] not in ("mcp", "izh"))
        else:
            np.savez_compressed(path, **out)
        print(name, "spikes per input:", [int(s["raster"].sum()) for s in snaps], "of", snaps[0]["raster"].size, "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
