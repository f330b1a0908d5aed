#!/usr/bin/env python3
"""Fixtures of Conv1dConnection / Conv3dConnection with PostPre: the UNMODIFIED reference's CPU path (build container only), one
thread, over the cases of tests/conv_nd_cases.py.  Per input: the Y raster (bit-packed), v, refrac_count, theta, the Y trace,
the X trace (as a sha256 where it has more than 5000 entries), w (in full for the small cases, as a sha256 for the others,
whose final w is stored once) and four draws of the global generator taken without moving it.  The initial weights are pinned
by the seed plus their sha256.

    python tests/golden/make_golden_conv_nd.py"""
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
import conv_nd_cases as CC  # noqa: E402
from dt_cases import save_fixture  # noqa: E402


def main(names=None):
    torch.set_num_threads(1)
    ns = CC.ns_from(ref_nodes, ref_topology, ref_learning, Network)
    for name in names or CC.CASES:
        net = CC.build(ns, name)
        w0 = CC.conn_of(net).w.detach().numpy().copy()
        snaps = CC.run_case(net, name, Monitor)
        out = {"w0_sha": np.array(CC.sha(w0)), "seed": np.array(CC.CASES[name]["seed"])}
        for r, s in enumerate(snaps):
            out[f"r{r}_raster"] = np.packbits(s["raster"].reshape(-1))
            out[f"r{r}_raster_sum"] = np.array(int(s["raster"].sum()))
            for k in ("v", "refrac", "theta", "xY", "gen"):
                out[f"r{r}_{k}"] = s[k]
            if s["xX"].size > 5000:
                out[f"r{r}_xX_sha"] = np.array(CC.sha(s["xX"]))
            else:
                out[f"r{r}_xX"] = s["xX"]
            out[f"r{r}_w_sha"] = np.array(CC.sha(s["w"]))
            if name not in CC.BIG:
                out[f"r{r}_w"] = s["w"]
        if name in CC.BIG and CC.CASES[name]["train"]:
            out["final_w"] = snaps[-1]["w"]
        path = os.path.join(HERE, f"convnd_{name}.npz")
        if "dt" in CC.CASES[name]:
            save_fixture(path, out, name, [s["raster"] for s in snaps], os.path.join(HERE, f"convnd_{CC.CASES[name]['sibling']}.npz"), refractory=True)
        else:
            np.savez_compressed(path, **out)
        print(name, "spikes per input:", [int(s["raster"].sum()) for s in snaps], "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1:])
