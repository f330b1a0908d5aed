#!/usr/bin/env python3
"""Fixtures of the real-valued (analog) Input: the UNMODIFIED reference's CPU path (build container only) over the cases of
tests/analog_cases.py, every Input driven by float32 values.  Writes tests/golden/analog_<case>.npz.

Per case and input: the bit-packed rasters of every non-Input layer, final v, refrac_count, x and summed, the pooling firing_rates,
and for the `tr_*` cases the Input's trace at every step.  A fixture is written only if
  * every non-Input layer's spike rate lies strictly between 0 and 1;
  * dyadic family: analog_cases.assert_dyadic holds, and the reference at 1 thread equals the reference at 8 threads equals the
    stated order (analog_cases.stated_run), bit for bit in every field;
  * float family: the stated order reproduces the reference's rasters, refrac_count and traces bit for bit, and every |v - thresh|
    met before a reset is at least MARGIN x v_spread, v_spread = max |reference - stated| over the per-step v; seeds are searched
    until that holds, and the seed, v_spread and summed_spread are stored.

    python tests/golden/make_golden_analog.py [case ...]"""
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
from bindsnet import conversion as ref_conversion  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import analog_cases as AC  # noqa: E402


def reference(ns, name, threads, seed=None):
    torch.set_num_threads(threads)
    try:
        return AC.run_case(ns, AC.build(ns, name, seed=seed, eval_mode=True), name)
    finally:
        torch.set_num_threads(1)


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def main(only):
    ns = AC.ns_from(ref_nodes, ref_topology, Network, Monitor, ref_conversion)
    ns.LIFNodes = ref_nodes.LIFNodes
    problems = []
    for name in AC.CASES:
        if only and name not in only:
            continue
        bad, out = [], {}
        if name not in AC.FLOAT:
            AC.assert_dyadic(name)
            snaps, snaps8, stated = reference(ns, name, 1), reference(ns, name, 8), AC.stated_run(name)
            for r, (a, b, c) in enumerate(zip(snaps, snaps8, stated)):
                for k in a:
                    if not same(a[k], b[k]):
                        bad.append((f"input {r} {k}: 1 thread != 8 threads", None))
                    if not same(a[k], np.asarray(c[k], a[k].dtype).reshape(a[k].shape)):
                        bad.append((f"input {r} {k}: stated order != reference", None))
            seed = AC.seed_of(name)
        else:
            for seed in range(AC.seed_of(name), AC.seed_of(name) + 4000, 100):
                snaps, stated = reference(ns, name, 1, seed=seed), AC.stated_run(name, seed=seed)
                v_spread = summed_spread = 0.0
                margin, exact = np.inf, True
                for a, b in zip(snaps, stated):
                    for k in a:
                        got = np.asarray(b[k], a[k].dtype).reshape(a[k].shape)
                        if k.endswith("_vrec") or k.endswith("_v"):
                            v_spread = max(v_spread, float(np.abs(a[k].astype(np.float64) - got).max()))
                        elif k.endswith("_summed"):
                            summed_spread = max(summed_spread, float(np.abs(a[k].astype(np.float64) - got).max()))
                        elif not same(a[k], got):
                            exact = False
                    margin = min([margin] + [v for k, v in b.items() if k.endswith("_margin")])
                print(f"    {name} seed {seed}: v_spread {v_spread:.3g}, summed_spread {summed_spread:.3g}, least |v - thresh| {margin:.3g}, "
                      f"rasters {'equal' if exact else 'DIFFER'}")
                if exact and margin >= AC.MARGIN * v_spread:
                    break
            else:
                bad.append(("no seed with the margin", None))
            out.update(v_spread=np.array(v_spread), summed_spread=np.array(summed_spread), least_margin=np.array(margin))
        out["seed"] = np.array(seed)
        for r, s in enumerate(snaps):
            for k, v in s.items():
                if k.endswith("_raster"):
                    rate = float(v.mean())
                    if not 0.0 < rate < 1.0:
                        bad.append((f"input {r} {k} rate", rate))
                if k.endswith("_vrec"):
                    continue                              # (per-step voltages: used for the spread, not stored)
                out[f"r{r}_{k}"] = np.packbits(v.reshape(-1)) if k.endswith("_raster") else v
        if any(not np.isfinite(a).all() for a in out.values() if a.dtype.kind == "f"):
            bad.append(("NaN or infinity", None))
        if bad:
            problems.append((name, bad))
            print(f"  {name}: NOT written: {bad[:4]}")
            continue
        path = os.path.join(HERE, f"analog_{name}.npz")
        np.savez_compressed(path, **out)
        rate = np.mean([v.mean() for s in snaps for k, v in s.items() if k.endswith("_raster")])
        print(f"  {name}: mean rate {rate:.3f}, {os.path.getsize(path)} bytes")
    assert not problems, problems


if __name__ == "__main__":
    main(set(sys.argv[1:]))
