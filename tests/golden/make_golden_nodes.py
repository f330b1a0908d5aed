#!/usr/bin/env python3
"""Fixtures of the node layers McCullochPitts / IFNodes / BoostedLIFNodes / CurrentLIFNodes / IzhikevichNodes: the UNMODIFIED
reference's CPU path (build container only) over the cases of tests/node_cases.py.  Per input: the Y raster (bit-packed), the
per-step v record (whole where small, else its sha256), and the final v, refrac_count, i, u, x -- whichever the layer has --
plus the Input trace and the weights of the connection cases.  Izhikevich cases also store r, a, b, c, d, S, excitatory.
nodes_ctor.npz: the seven Izhikevich buffers and the generator state the constructor leaves, per (seed, n, excitatory).

    python tests/golden/make_golden_nodes.py"""
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
from bindsnet.network import nodes as ref_nodes, topology as ref_topology, topology_features as ref_features  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import node_cases as NC  # noqa: E402
from dt_cases import save_fixture  # noqa: E402

VREC_WHOLE = 2500          # per-step v records of at most this many floats are stored whole


def main():
    torch.set_num_threads(1)
    ns = NC.ns_from(ref_nodes, ref_topology, ref_features, ref_mcc_learning, Network)
    problems = []
    for name, c in NC.CASES.items():
        net = NC.build(ns, name)
        out = {"seed": np.array(c["seed"])}
        if c["kind"] == "izh":
            for k in NC.IZH_BUFFERS:
                out[k] = getattr(net.layers["Y"], k).numpy().copy()
        if c["graph"] == "mcc":
            out["w0_sha"] = np.array(NC.sha(NC.weights(net).detach().numpy()))
        snaps = NC.run_case(net, name, Monitor)
        per_step = []
        for r, s in enumerate(snaps):
            out[f"r{r}_raster"] = np.packbits(s["raster"].reshape(-1))
            out[f"r{r}_raster_sum"] = np.array(int(s["raster"].sum()))
            out[f"r{r}_vrec_sha"] = np.array(NC.sha(s["vrec"]))
            if s["vrec"].size <= VREC_WHOLE:
                out[f"r{r}_vrec"] = s["vrec"]
            for k in NC.STATE + ("xX", "w"):
                if k in s:
                    out[f"r{r}_{k}"] = s[k]
            per_step.append(s["raster"].sum(axis=2))                 # [T, B] spikes per step and sample
        counts = np.concatenate(per_step).reshape(-1)
        if c["kind"] == "izh" and c["graph"] == "direct":
            # both branches of the lateral sum (k < 8: scalar row_sum; k >= 8: 8-lane vectors) must be exercised
            if not (((counts > 0) & (counts < 8)).any() and (counts >= 8).any()):
                problems.append((name, "spike counts per step do not cross 8", sorted(set(counts.tolist()))))
        total = int(sum(s["raster"].sum() for s in snaps))
        cells = sum(s["raster"].size for s in snaps)
        if not 0.005 < total / cells < 0.7:                          # neither empty nor saturated
            problems.append((name, "spike rate", total / cells))
        path = os.path.join(HERE, f"nodes_{name}.npz")
        if "dt" in c:           # (McCullochPitts and IzhikevichNodes have no refractory period)
            save_fixture(path, out, name, [s["raster"] for s in snaps], os.path.join(HERE, f"nodes_{c['sibling']}.npz"),
                         refractory=c["kind"] in ("if", "boosted", "clif"), also=[s["vrec"] for s in snaps])
        else:
            np.savez_compressed(path, **out)
        print(name, "spikes per input:", [int(s["raster"].sum()) for s in snaps], "rate %.3f" % (total / cells),
              "per-step spike counts min/max:", int(counts.min()), int(counts.max()), "bytes:", os.path.getsize(path))

    assert not problems, problems
    out = {}
    for seed, n, exc in NC.CTOR:
        torch.manual_seed(seed)
        layer = ref_nodes.IzhikevichNodes(n=n, excitatory=exc)
        for k in NC.IZH_BUFFERS:
            out[f"s{seed}_{k}"] = getattr(layer, k).numpy().copy()
        out[f"s{seed}_rng"] = torch.get_rng_state().numpy().copy()
        out[f"s{seed}_v"], out[f"s{seed}_u"] = layer.v.numpy().copy(), layer.u.numpy().copy()
    path = os.path.join(HERE, "nodes_ctor.npz")
    np.savez_compressed(path, **out)
    print("ctor bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
