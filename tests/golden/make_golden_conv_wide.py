#!/usr/bin/env python3
"""Fixtures of Conv2dConnection with more than 16 input channels: the UNMODIFIED reference's CPU path (build container only), one
thread, over the cases of tests/conv_wide_cases.py.  Writes tests/golden/conv_wide_<case>.npz.

Per case and input: the bit-packed raster of every non-Input layer, v / refrac_count / x / summed of the spiking layers and the
pooling firing_rates in full, the sha256 of every initial `w` and `b`.  A fixture is written only if
  * every spiking layer fires on more than 2 % and fewer than 40 % of its neuron-steps (a silent or saturated fixture would pass
    for parity whatever the sums are);
  * the reference at 8 threads equals the reference at 1 thread bit for bit in every field (the sums are exact on the 1/64 grid,
    so no order or blocking can change them);
  * nothing stored is NaN or infinite.

    python tests/golden/make_golden_conv_wide.py [case ...]"""
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
import conv_wide_cases as WC  # noqa: E402


def reference(ns, name, threads):
    torch.set_num_threads(threads)
    try:
        net = WC.build(ns, name, eval_mode=True)
        shas = WC.weights_sha(net)
        return WC.run_case(ns, net, name), shas, net
    finally:
        torch.set_num_threads(1)


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def main(only):
    torch.set_num_threads(1)
    ns = WC.ns_from(ref_nodes, ref_topology, Network, Monitor, ref_conversion)
    for name in WC.NAMES:
        if only and name not in only:
            continue
        snaps, shas, net = reference(ns, name, 1)
        snaps8, shas8, _ = reference(ns, name, 8)
        assert shas == shas8
        assert WC.wide(net), f"case {name} has no convolution with more than 16 input channels"
        for r, (a, b) in enumerate(zip(snaps, snaps8)):
            for k in a:
                assert same(a[k], b[k]), f"case {name} input {r} {k}: 1 thread != 8 threads"
        rates = {}
        for l in WC.spiking_layers(net):
            rates[l] = float(np.mean([s[f"{l}_raster"].mean() for s in snaps]))
            assert WC.RATE_BAND[0] < rates[l] < WC.RATE_BAND[1], f"case {name}: layer {l} fires on {rates[l]:.4f} of its neuron-steps"
        out = {"weights_sha": np.array(shas)}
        for r, s in enumerate(snaps):
            for k, v in s.items():
                out[f"r{r}_{k}"] = np.packbits(v.reshape(-1)) if k.endswith("_raster") else v
        assert all(np.isfinite(a).all() for a in out.values() if a.dtype.kind == "f"), f"case {name}: NaN or infinity"
        path = os.path.join(HERE, f"conv_wide_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"  {name}: rates {', '.join(f'{l} {v:.3f}' for l, v in rates.items())}; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(set(sys.argv[1:]))
