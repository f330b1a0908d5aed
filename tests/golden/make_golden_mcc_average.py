#!/usr/bin/env python3
"""Fixtures of the time-averaged MCC rules (average_update / continues_update): the UNMODIFIED reference's CPU path, one thread
(build container only), over the cases of tests/mcc_average_cases.py.  Writes tests/golden/mcc_average_<rule>_b<B>_<w|c>.npz: per case and
input the packed Y raster, W, the rings, the ring indices and the rule's state.

A fixture is written only if mcc_average_cases.conditions holds for every case on the reference's own output: the output layer
spikes, W moves, W differs from the plain rule's for every K > 1 (and equals it bit for bit at K = 1), the two modes differ, a clamp
bound binds, and the ring is non-zero at the end of input 1 (so its persistence across reset_state_variables() is exercised).

    python tests/golden/make_golden_mcc_average.py"""
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
from bindsnet.learning import MCC_learning as ref_mcc  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology, topology_features as ref_features  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import mcc_average_cases as AC  # noqa: E402

NS = AC.ns_from(ref_nodes, ref_topology, ref_features, ref_mcc, Network, Monitor)


def main():
    warnings.simplefilter("ignore")
    torch.set_num_threads(1)
    files = {}
    for case, c in AC.CASES.items():
        got = AC.run(NS, AC.build(NS, case), case)
        plain = AC.run(NS, AC.build(NS, case, K=0), case)
        other = AC.run(NS, AC.build(NS, case, cont=not c["cont"]), case)
        pre_norm = AC.run(NS, AC.build(NS, case, norm=False), case, n_in=1)
        AC.conditions(case, got, plain, other, pre_norm)
        for ring, index in AC.RINGS[c["rule"]]:
            moved = c.get("nu", (1, 1))[0] != 0.0 or not ring.endswith("_pre")
            assert int(got[-1][index]) == ((AC.INPUTS * AC.T) % c["K"] if moved else 0), (case, index)
        files.setdefault(AC.fixture_of(case), {}).update(AC.pack(case, got))
        print(case, [int(g["raster"].sum()) for g in got], "spikes")
    for name, arrays in files.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        print(name, len(arrays), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
