#!/usr/bin/env python3
"""Fixtures of SparseConnection: the UNMODIFIED reference's CPU path (build container only), one thread, over the cases of
tests/sparse_cases.py.  Per input: the Y raster (bit-packed), v, refrac_count, theta (DiehlAndCookNodes), the traces (as a sha256
where one has more than 5000 entries) and four draws of the global generator taken without moving it.  The initial weights are
pinned by the seed plus the sha256 of every connection's dense weights, in connection order.

    python tests/golden/make_golden_sparse.py"""
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
from bindsnet.network import nodes as ref_nodes, topology as ref_topology  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import sparse_cases as SC  # noqa: E402
from dt_cases import save_fixture  # noqa: E402


def main(names=None):
    torch.set_num_threads(1)
    ns = SC.ns_from(ref_nodes, ref_topology, Network)
    for name in names or SC.CASES:
        net = SC.build(ns, name)
        assert all(c.w.is_sparse for c in net.connections.values())
        out = {"w0_sha": np.array(SC.weights_sha(net)), "w0_nnz": np.array([int(c.w._nnz()) for c in net.connections.values()]),
               "seed": np.array(SC.CASES[name]["seed"])}
        snaps = SC.run_case(net, name, Monitor)
        for r, s in enumerate(snaps):
            out[f"r{r}_raster"] = np.packbits(s.pop("raster").reshape(-1))
            for k, v in s.items():
                if v.size > 5000:
                    out[f"r{r}_{k}_sha"] = np.array(SC.sha(v))
                else:
                    out[f"r{r}_{k}"] = v
        path = os.path.join(HERE, f"sparse_{name}.npz")
        c = SC.CASES[name]
        if "dt" in c:
            rasters = [np.unpackbits(out[f"r{r}_raster"])[:c["T"] * c["B"] * c["n"]].reshape(c["T"], c["B"], c["n"]) for r in range(len(snaps))]
            save_fixture(path, out, name, rasters, os.path.join(HERE, f"sparse_{c['sibling']}.npz"), refractory=True)
        else:
            np.savez_compressed(path, **out)
        print(name, "spikes per input:", [int(np.unpackbits(out[f"r{r}_raster"]).sum()) for r in range(len(snaps))], "nnz:",
              out["w0_nnz"].tolist(), "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1:])
