#!/usr/bin/env python3
"""Fixtures of CSRMNodes: the UNMODIFIED reference's CPU path (build container only) over the cases of tests/csrm_cases.py, one
thread.  Per case and input: the Y raster (bit-packed), v, theta, last_spikes, the X -> Y window s_w, both traces and w; per case
the seed, `v_spread` and `min_margin`.

The device cannot follow torch's einsum and matmul (blocked BLAS orders) bit for bit; it follows the order stated in
tests/csrm_cases.py.  For every case the generator runs that stated order beside the reference and measures
    v_spread   = max |v_reference - v_stated_order|  over all inputs, steps, samples and neurons,
    min_margin = min |v - (thresh + theta)|          of the reference run, at the moment of the comparison.
A fixture is written for the FIRST seed (ascending from 0, at most csrm_cases.MAX_SEEDS) whose reference run keeps min_margin >=
MARGIN_FACTOR * v_spread: then no spike can hinge on the order, and the raster, theta, last_spikes, s_w, the traces and the learned
weights of the stated order must be -- and are checked here to be -- the reference's bit for bit.  A case without such a seed fails.

A second table, csrm_raises.json, holds the exception type of every call of csrm_cases.RAISING in the reference.

    python tests/golden/make_golden_csrm.py [case ...]"""
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
from bindsnet.learning import learning as ref_learning  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import csrm_cases as CC  # noqa: E402

DISCRETE = ("raster", "theta", "last", "s_w", "xX", "xY", "w")


def hook(layer, rec):
    """Record, per forward(): v behind the step and the least distance of any v from its threshold at the comparison."""
    orig = layer.forward

    def forward(x):
        thr = layer.thresh + (layer.theta * layer.theta_decay if layer.learning else layer.theta)
        orig(x)
        # (lbound lies far below every threshold: a clipped v is nearer to it than the v that was compared, never across it)
        rec["margin"] = min(rec["margin"], float((layer.v.double() - thr.double()).abs().min()))
        assert torch.equal(layer.v >= thr, layer.s)
        rec["v"].append(layer.v.numpy().copy())

    layer.forward = forward


def attempt(ns, c, seed):
    net = CC.build(ns, c, seed)
    rec = {"margin": np.inf, "v": []}
    hook(net.layers["Y"], rec)
    snaps = CC.run_case(net, c, seed, Monitor)
    Y = net.layers["Y"]
    stated = CC.stated_run(c, seed, record_v=True, decays=(Y.decay.numpy(), Y.theta_decay.numpy()))
    v_ref = np.stack(rec["v"]).reshape(c["n_in"], c["T"], c["B"], c["N"])
    spread = max(float(np.abs(v_ref[r].astype(np.float64) - stated[r]["vrec"].astype(np.float64)).max()) for r in range(c["n_in"]))
    return net, snaps, stated, spread, rec["margin"]


def main(only):
    torch.set_num_threads(1)
    warnings.simplefilter("ignore")
    ns = CC.ns_from(ref_nodes, ref_topology, ref_learning, Network)
    for name, c in CC.CASES.items():
        if only and name not in only:
            continue
        for seed in range(CC.MAX_SEEDS):
            net, snaps, stated, spread, margin = attempt(ns, c, seed)
            if margin >= CC.MARGIN_FACTOR * spread:
                break
        else:
            raise SystemExit(f"{name}: none of the first {CC.MAX_SEEDS} seeds keeps every |v - threshold| >= {CC.MARGIN_FACTOR} v_spread")
        out = {"seed": np.array(seed), "v_spread": np.array(spread), "min_margin": np.array(margin),
               "decay": net.layers["Y"].decay.numpy().copy(), "theta_decay": net.layers["Y"].theta_decay.numpy().copy(), "resKernel": net.layers["Y"].resKernel.numpy().copy(),
               "refKernel": net.layers["Y"].refKernel.numpy().copy()}
        rate = float(np.mean([s["raster"].mean() for s in snaps]))
        assert 0.005 < rate < 0.7, (name, "spike rate", rate)
        for r, (s, q) in enumerate(zip(snaps, stated)):
            for k in DISCRETE:
                assert s[k].shape == q[k].shape and np.array_equal(s[k], q[k]), (name, r, k, "stated order differs from the reference")
            assert np.abs(s["v"] - q["v"]).max() <= spread
            for k, a in s.items():
                out[f"r{r}_{k}"] = np.packbits(a.reshape(-1)) if k == "raster" else a
        assert net.layers["Y"].last_spikes.dtype == torch.float32 and net.connections[("X", "Y")].s_w.dtype == torch.float32
        if c["rule"]:
            moved = float(np.abs(snaps[-1]["w"] - CC.weights(c, seed)["w"].numpy()).max())
            assert moved > 1e-3, (name, "largest weight movement", moved)
        path = os.path.join(HERE, f"csrm_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"  {name}: seed {seed}, rate {rate:.3f}, |v| <= {max(np.abs(s['v']).max() for s in snaps):.1f}, v_spread {spread:.3g}, "
              f"min margin {margin:.3g}, {os.path.getsize(path)} bytes")
    if not only:
        table = {}
        for name, call in CC.RAISING.items():
            try:
                call(ns)
                table[name] = None
            except BaseException as e:                     # noqa: BLE001
                table[name] = type(e).__name__
            print(f"  raises {name}: {table[name]}")
        with open(os.path.join(HERE, "csrm_raises.json"), "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main(set(sys.argv[1:]))
