#!/usr/bin/env python3
"""Fixtures of the MulticompartmentConnection feature pipelines (Probability / Mask / Weight / Bias / Intensity): the UNMODIFIED
reference's CPU path (build container only), one thread, over the cases of tests/mcc_pipe_cases.py.  Per case and input: every
non-input layer's raster (bit-packed) and spike count, the final v / refrac_count / traces / theta, the sha256 of every feature
value (the values themselves after the last input, and after every input where a rule or a norm changes them) and
torch.get_rng_state(); plus the generator state after construction and the number of 32-bit draws each input consumed.
mccpipe_ctor.npz: value=None constructions and the exception type of every raising constructor call.

    python tests/golden/make_golden_mcc_pipe.py"""
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
from bindsnet import models as ref_models  # noqa: E402
from bindsnet.learning import MCC_learning as ref_mcc_learning  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology, topology_features as ref_features  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import mcc_pipe_cases as PC  # noqa: E402
from dt_cases import save_fixture  # noqa: E402


def draws_between(state0, state1, limit):
    """Number of 32-bit outputs that take the generator from state0 to state1 (searched up to `limit`)."""
    keep = torch.get_rng_state()
    torch.set_rng_state(torch.from_numpy(state0.copy()))
    n, step = 0, 1
    want = torch.from_numpy(state1)
    g = torch.default_generator
    while n <= limit:
        if torch.equal(torch.get_rng_state(), want):
            torch.set_rng_state(keep)
            return n
        torch.empty(step, dtype=torch.int32).random_(generator=g)          # one 32-bit output per element
        n += step
    torch.set_rng_state(keep)
    return -1


def main():
    torch.set_num_threads(1)
    ns = PC.ns_from(ref_nodes, ref_topology, ref_features, ref_mcc_learning, Network, ref_models)
    problems = []
    for name, c in PC.CASES.items():
        net = PC.build(ns, name)
        out = {"seed": np.array(c["seed"]), "rng_ctor": torch.get_rng_state().numpy().copy()}
        learned = {k for k, v in PC.features(net).items() if c.get("rule") or c["graph"] == "dc"}
        before = out["rng_ctor"]
        snaps = PC.run_case(net, name, Monitor)
        total = 0
        per_step = sum(conn.source.n * conn.target.n for conn in net.connections.values() for f in conn.pipeline
                       if type(f).__name__ == "Probability")
        for r, s in enumerate(snaps):
            for k, v in s.items():
                if k.startswith("raster_"):
                    out[f"r{r}_{k}"] = np.packbits(v.reshape(-1))
                    out[f"r{r}_{k}_sum"] = np.array(int(v.sum()))
                    total += int(v.sum())
                elif k.startswith("feat_"):
                    out[f"r{r}_{k}_sha"] = np.array(PC.sha(v))
                    if r == len(snaps) - 1 or k[5:] in learned:
                        out[f"r{r}_{k}"] = v
                else:
                    out[f"r{r}_{k}"] = v
            n = draws_between(before, s["rng"], c["T"] * per_step + 200000)
            out[f"r{r}_draws"] = np.array(n)
            if c["graph"] != "dc" and n != c["T"] * per_step:
                problems.append((name, r, "draws", n, c["T"] * per_step))
            before = s["rng"]
        out["spikes"] = np.array(total)
        if total < PC.MIN_SPIKES:
            problems.append((name, "spikes", total))
        path = os.path.join(HERE, f"mccpipe_{name}.npz")
        if "dt" in c:
            rasters = [v for s in snaps for k, v in s.items() if k.startswith("raster_")]
            save_fixture(path, out, name, rasters, os.path.join(HERE, f"mccpipe_{c['sibling']}.npz"), refractory=True)
        else:
            np.savez_compressed(path, **out)
        print(name, "spikes:", {k: int(v) for k, v in out.items() if k.endswith("_sum")}, "draws:", [int(out[f"r{r}_draws"]) for r in range(len(snaps))],
              "bytes:", os.path.getsize(path))
    out = {}
    for seed, letter, S, N in PC.CTOR:
        for k, v in PC.ctor_case(ns, seed, letter, S, N).items():
            out[f"s{seed}_{k}"] = v
        print("ctor", letter, {k: (v.dtype, v.shape) if k != "raises" else str(v) for k, v in PC.ctor_case(ns, seed, letter, S, N).items()})
    for rname, call in PC.raising_cases().items():
        try:
            call(ns)
            out[f"raise_{rname}"] = np.array("")
        except Exception as e:               # noqa: BLE001
            out[f"raise_{rname}"] = np.array(type(e).__name__)
        print("raise", rname, str(out[f"raise_{rname}"]))
    # [Mask] alone: the reference's integer sum, added into the float input
    torch.manual_seed(3)
    X, Y = ns.Input(n=6), ns.LIFNodes(n=5)
    m = np.random.default_rng(3).random((6, 5)) < 0.6
    conn = ns.MulticompartmentConnection(X, Y, device="cpu", pipeline=[ns.Mask("m", torch.from_numpy(m))])
    s = torch.from_numpy((np.random.default_rng(4).random((2, 6)) < 0.5).astype(np.uint8))
    res = conn.compute(s)
    out["mask_alone_mask"], out["mask_alone_s"], out["mask_alone_out"] = m, s.numpy(), res.numpy()
    out["mask_alone_dtype"] = np.array(str(res.dtype))
    print("mask alone:", res.dtype, res.tolist())
    path = os.path.join(HERE, "mccpipe_ctor.npz")
    np.savez_compressed(path, **out)
    print("ctor bytes:", os.path.getsize(path))
    assert not problems, problems


if __name__ == "__main__":
    main()
