#!/usr/bin/env python3
"""Fixtures of the locally connected family (LocalConnection1D / 2D / 3D with PostPre, AdaptiveLIFNodes): the UNMODIFIED
reference's CPU path (build container only) over the cases of tests/local_cases.py.  Per input: the Y raster (bit-packed),
v, refrac_count, theta, both traces, and w -- in full for the small cases, as a sha256 for the 64 800-weight loc2d graph
(whose final w is stored once).  The initial weights are pinned by the seed plus their sha256.

    python tests/golden/make_golden_local.py"""
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
from bindsnet.learning import learning as ref_learning  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import local_cases as LC  # noqa: E402
from dt_cases import save_fixture  # noqa: E402

BIG = ("a", "e")


def main():
    torch.set_num_threads(1)
    ns = LC.ns_from(ref_nodes, ref_topology, ref_learning, Network)
    for name in LC.CASES:
        net = LC.build(ns, name)
        w0 = LC.w_of(net).detach().numpy().copy()
        snaps = LC.run_case(net, name, Monitor)
        out = {"w0_sha": np.array(LC.sha(w0)), "seed": np.array(LC.CASES[name]["seed"])}
        for r, s in enumerate(snaps):
            out[f"r{r}_raster"] = np.packbits(s["raster"].reshape(-1))
            out[f"r{r}_raster_sum"] = np.array(int(s["raster"].sum()))
            for k in ("v", "refrac", "theta", "xX", "xY"):
                out[f"r{r}_{k}"] = s[k]
            out[f"r{r}_w_sha"] = np.array(LC.sha(s["w"]))
            if name not in BIG:
                out[f"r{r}_w"] = s["w"]
        if name in BIG:
            out["final_w"] = snaps[-1]["w"]
        path = os.path.join(HERE, f"local_{name}.npz")
        if "dt" in LC.CASES[name]:
            save_fixture(path, out, name, [s["raster"] for s in snaps], os.path.join(HERE, f"local_{LC.CASES[name]['sibling']}.npz"), refractory=True)
        else:
            np.savez_compressed(path, **out)
        print(name, "spikes per input:", [int(s["raster"].sum()) for s in snaps], "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
