#!/usr/bin/env python3
"""Fixtures of Hebbian / WeightDependentPostPre on a Conv2dConnection: the UNMODIFIED reference's CPU path (build container only)
over the cases of tests/conv2d_rule_cases.py, single-threaded.  Per input: the Y raster (bit-packed), v, refrac_count, both traces
and w.  The generator fails when a case has no output spike or when w does not move while learning is on.

    python tests/golden/make_golden_conv2d_rules.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import stage_ref  # noqa: E402
REF = stage_ref.REF_ROOT
for name, path in (("bindsnet", REF), ("bindsnet.analysis", REF + "/analysis")):
    pkg = types.ModuleType(name)
    pkg.__path__ = [path]
    sys.modules[name] = pkg
sys.modules["cv2"] = types.ModuleType("cv2")
import tv_shim  # noqa: E402
tv_shim.install()
import bindsnet.network  # noqa: E402,F401  (first, like the reference's own import order)
from bindsnet.learning import learning as ref_learning  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import conv2d_rule_cases as CC  # noqa: E402
from dt_cases import save_fixture  # noqa: E402


def main():
    torch.set_num_threads(1)
    ns = CC.ns_from(ref_nodes, ref_topology, ref_learning, Network)
    for name, c in CC.CASES.items():
        assert np.prod(CC.out_hw(c)) <= 64, name
        net = CC.build(ns, name)
        w0 = CC.w_of(net).detach().numpy().copy()
        snaps = CC.run_case(net, name, Monitor)
        spikes = [int(s["raster"].sum()) for s in snaps]
        assert all(n > 0 for n in spikes), f"{name}: an input without an output spike {spikes}"
        moved = [not np.array_equal(a, b) for a, b in zip([w0] + [s["w"] for s in snaps[:-1]], [s["w"] for s in snaps])]
        assert all(m == c["train"] for m in moved), f"{name}: weights moved per input {moved}, learning {c['train']}"
        out = {"w0_sha": np.array(CC.sha(w0)), "seed": np.array(c["seed"])}
        for r, s in enumerate(snaps):
            out[f"r{r}_raster"] = np.packbits(s["raster"].reshape(-1))
            out[f"r{r}_raster_sum"] = np.array(spikes[r])
            for k in ("v", "refrac", "xX", "xY", "w"):
                out[f"r{r}_{k}"] = s[k]
        path = CC.gold_path(name)
        if "dt" in c:
            save_fixture(path, out, name, [s["raster"] for s in snaps], CC.gold_path(c["sibling"]), refractory=True)
        else:
            np.savez_compressed(path, **out)
        print(name, "spikes per input:", spikes, "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
