#!/usr/bin/env python3
"""Fixtures of the float16 / bfloat16 Weight features: the UNMODIFIED reference's CPU path at one thread (build container only)
over the cases of tests/half_cases.py -- DiehlAndCook2015(w_dtype=torch.float16 | torch.bfloat16).  Per input: the Ae and Ai
rasters (bit-packed), v and refrac_count of both layers, theta, both traces, the learned X -> Ae value as raw uint16 patterns and
the sha256 of the global generator's state (one_spike draws from it).  Only data is written: tests/golden/half_<case>.npz.

A case is kept only if the reference alone shows that it exercises what it is for: every input makes Ae spike, and in the
training cases the value changes from every input to the next (and from its initial state).

    python tests/golden/make_golden_half.py"""
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
from bindsnet.models import models as ref_models  # noqa: E402
from bindsnet.network import monitors as ref_monitors  # noqa: E402
import half_cases as HC  # noqa: E402

FLOATS = ("vE", "vI", "theta", "refracE", "refracI", "xX", "xE")


def main():
    torch.set_num_threads(1)
    ns = HC.ns_from(ref_models, ref_monitors)
    for name in sorted(HC.CASES):
        net = HC.build(ns, name)
        assert HC.value_of(net).dtype == HC.dtype_of(name)
        v0 = HC.bits16(HC.value_of(net))
        snaps = HC.run_case(net, name, ref_monitors.Monitor)
        out = {"seed": np.array(HC.CASES[name]["seed"]), "value0_sha": np.array(HC.sha(v0))}
        prev = v0
        for r, s in enumerate(snaps):
            assert s["sE"].sum() > 0, f"case {name}: input {r} makes no Ae neuron spike"
            if HC.CASES[name]["train"]:
                assert not np.array_equal(s["value"], prev), f"case {name}: the value does not change over input {r}"
            prev = s["value"]
            for k in ("sE", "sI"):
                out[f"r{r}_{k}"] = np.packbits(s[k].reshape(-1))
                out[f"r{r}_{k}_sum"] = np.array(int(s[k].sum()))
            for k in FLOATS:
                assert np.isfinite(s[k]).all(), f"case {name}: {k} of input {r} is not finite"
                out[f"r{r}_{k}"] = s[k]
            out[f"r{r}_value"] = s["value"]
            out[f"r{r}_rng_sha"] = np.array(HC.sha(s["rng"]))
        path = os.path.join(HERE, f"half_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, "Ae spikes per input:", [int(s["sE"].sum()) for s in snaps], "Ai:", [int(s["sI"].sum()) for s in snaps],
              "changed weights per input:", [int((a["value"] != b).sum()) for a, b in zip(snaps, [v0] + [s["value"] for s in snaps[:-1]])],
              "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
