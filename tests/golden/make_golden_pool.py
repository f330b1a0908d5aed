#!/usr/bin/env python3
"""Fixtures of MaxPool1d / 2d / 3dConnection and MeanFieldConnection: the UNMODIFIED reference's CPU path (build container only),
one thread, over the cases of tests/pool_cases.py.  Per input: the target raster (bit-packed), the target's v, refrac_count and
trace, the pooling connection's firing_rates and, for case h, the convolution's learned weights.  Per pooling case the share of
window decisions that picked a tap other than the window's first in-bounds one and the share of windows that hold their maximum
more than once, both asserted to be substantial: a fixture in which the first tap always won would not tell the index rule from
"take the first tap".  Every decision is also checked against tests/pool_cases.py's own window enumeration.

Case h runs in training mode, which the reference's pooling classes cannot (NoOp multiplies a `w` they do not have): the generator
gives the reference's pooling OBJECT a dummy attribute from outside, `pool.w = torch.zeros(())`; no reference code is changed.

pool_ctor.npz: per MeanFieldConnection constructor variant its `w`, the rule's weight_decay and the generator's position behind the
constructor; and what every call of pool_cases.CALLS does in the reference ("ok" or the exception's class name).

    python tests/golden/make_golden_pool.py"""
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
from bindsnet import learning as ref_learning  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import pool_cases as PC  # noqa: E402
from dt_cases import save_fixture  # noqa: E402


def watch(conn, geom, tally):
    """Count, at every compute() of the reference's pooling object, the decisions of its windows."""
    taps = PC.window_taps(geom)
    pool = getattr(torch.nn.functional, f"max_pool{geom['nd']}d")
    inner = conn.compute

    def compute(s):
        out = inner(s)
        fr = conn.firing_rates
        idx, nonfirst, ties, n = PC.window_stats(fr.numpy(), taps)
        _, ref_idx = pool(fr, kernel_size=conn.kernel_size, stride=conn.stride, padding=conn.padding, dilation=conn.dilation,
                          return_indices=True)
        assert np.array_equal(idx.reshape(-1), ref_idx.numpy().reshape(-1)), "the first-maximum rule is not what torch returned"
        tally[:] += np.array([nonfirst, ties, n])
        return out
    conn.compute = compute


def main(names=None):
    torch.set_num_threads(1)
    ns = PC.ns_from(ref_nodes, ref_topology, Network, ref_learning)
    for name in names or PC.CASES:
        net = PC.build(ns, name)
        out = {"seed": np.array(PC.seed_of(name))}
        pool, tally = PC.pool_of(net), np.zeros(3, np.int64)
        if pool is not None:
            geom = PC.POOL[name] if name in PC.POOL else dict(nd=2, shape=tuple(pool.source.shape), k=2, s=2, p=0, d=1)
            watch(pool, geom, tally)
            if net.learning:
                pool.w = torch.zeros(())               # lets the unmodified NoOp.update run (see the docstring)
        for key, conn in net.connections.items():
            if hasattr(conn, "w") and conn is not pool:
                out["w0_" + "_".join(key)] = conn.w.detach().numpy().astype(np.float32)
        snaps = PC.run_case(net, name, Monitor)
        for r, s in enumerate(snaps):
            out[f"r{r}_raster"] = np.packbits(s.pop("raster").reshape(-1))
            for k, v in s.items():
                out[f"r{r}_{k}"] = v
        if pool is not None:
            out["share_nonfirst"], out["share_ties"] = tally[0] / tally[2], tally[1] / tally[2]
            assert out["share_nonfirst"] >= 0.10 and out["share_ties"] > 0.0, (name, tally)
        path = os.path.join(HERE, f"pool_{name}.npz")
        if name in PC.DT:
            T, B = PC.steps_of(name), PC.batch_of(name)
            rasters = [np.unpackbits(out[f"r{r}_raster"]).reshape(-1)[:T * B * net.layers["Y"].n].reshape(T, B, -1) for r in range(len(snaps))]
            save_fixture(path, out, name, rasters, os.path.join(HERE, f"pool_{PC.base(name)}.npz"), refractory=True)
        else:
            np.savez_compressed(path, **out)
        print(name, "spikes per input:", [int(np.unpackbits(out[f"r{r}_raster"]).sum()) for r in range(len(snaps))],
              "not-first / tie shares:", None if pool is None else (round(float(out["share_nonfirst"]), 3), round(float(out["share_ties"]), 3)),
              "bytes:", os.path.getsize(path))
    if names:
        return
    out = {}
    for variant in PC.CTOR:
        conn, probe = PC.ctor(ns, variant)
        out[f"{variant}_w"] = conn.w.detach().numpy().astype(np.float32)
        out[f"{variant}_gen"] = probe
        out[f"{variant}_rule_decay"] = np.array(float(conn.update_rule.weight_decay))
    out["calls"] = np.array(sorted(PC.CALLS))
    out["outcomes"] = np.array([PC.outcome(ns, call) for call in sorted(PC.CALLS)])
    np.savez_compressed(os.path.join(HERE, "pool_ctor.npz"), **out)
    print({c: o for c, o in zip(out["calls"].tolist(), out["outcomes"].tolist())})


if __name__ == "__main__":
    main(sys.argv[1:])
