#!/usr/bin/env python3
"""Fixtures of the state monitors (x, theta, refrac_count, i of layers; `activity` of MulticompartmentConnection(traces=True)): the
UNMODIFIED reference's CPU path (build container only), one thread, over the cases of tests/state_monitor_cases.py.  Per case and
input: everything the case's monitors recorded (spike records bit-packed), the layers' final state, every feature value and
torch.get_rng_state().  No record may be vacuous: the generator demands spikes, a positive theta, a running refractory counter, a
non-zero synaptic current and a non-zero activity of the reference's own run, wherever the case records them.

    python tests/golden/make_golden_state_monitors.py"""
import os
import sys
import types

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
from bindsnet.network import monitors as ref_monitors, nodes as ref_nodes, topology as ref_topology, topology_features as ref_features  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import state_monitor_cases as SC  # noqa: E402


def main():
    torch.set_num_threads(1)
    ns = SC.ns_from(ref_nodes, ref_topology, ref_features, ref_mcc_learning, Network, ref_monitors)
    problems = []
    for name, c in SC.CASES.items():
        net = SC.build(ns, name)
        out = {"seed": np.array(c["seed"])}
        for r, snap in enumerate(SC.run_case(ns, net, name)):
            for k, v in snap.items():
                if k.endswith("_s") and (k.startswith("rec_") or k.startswith("net_")):
                    out[f"r{r}_{k}"] = np.packbits(v.astype(np.uint8).reshape(-1))
                    out[f"r{r}_{k}_shape"] = np.array(v.shape)
                    if k.endswith("Y_s") and v.sum() < 20:
                        problems.append((name, r, k, "spikes", int(v.sum())))
                else:
                    out[f"r{r}_{k}"] = v
                recorded = k.startswith(("rec_", "net_", "act_"))
                if recorded and k.endswith("_theta") and not (v > 0).any():
                    problems.append((name, r, k, "theta never positive"))
                if recorded and k.endswith(("_refrac_count", "_i", "_x")) and not (v != 0).any():
                    problems.append((name, r, k, "all zero"))
                if k.startswith("act_") and not (v != 0).any():
                    problems.append((name, r, k, "activity all zero"))
                if recorded and v.dtype.kind == "f" and not np.isfinite(v).all():
                    problems.append((name, r, k, "not finite"))
            if not any(k.endswith("Y_s") for k in snap):
                problems.append((name, r, "no spike record of Y"))
        path = os.path.join(HERE, f"state_monitors_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, {k: v.shape for k, v in out.items() if k.startswith("r0_") and not k.endswith("_shape")}, "bytes:", os.path.getsize(path))
    assert not problems, problems


if __name__ == "__main__":
    main()
