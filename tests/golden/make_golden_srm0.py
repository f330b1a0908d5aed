#!/usr/bin/env python3
"""Fixtures of SRM0Nodes and Rmax: the UNMODIFIED reference's CPU path (build container only) over the cases of tests/srm0_cases.py,
one thread.  Per case and input, per SRM0 layer L: the raster (bit-packed), the per-step v and s_prob, the per-step uniform draws
(recovered by replaying torch.rand_like from the generator state saved in front of the layer's forward()), the final v,
refrac_count, x and s_prob; the Input trace and the weights of the connection cases; for the Rmax cases the per-step source trace
and the final eligibility_trace; the 5056-byte generator state before and after the input.

A fixture is written only if the reference's own record meets every condition -- a case that misses one gets another seed in
tests/srm0_cases.py, never a waiver:
  * the spike rate lies in (0.005, 0.7);
  * every draw is at least srm0_cases.MARGIN away from its s_prob (2^-20; 2^-14 in the Rmax cases), so that a few ulp of
    difference between two exponential functions cannot flip a spike; the least margin found is stored (`min_margin`);
  * in the Rmax cases fewer than 5 % of the weights sit on a bound at the end, and the weights moved.

    python tests/golden/make_golden_srm0.py [case ...]"""
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
from bindsnet.network import nodes as ref_nodes, topology as ref_topology, topology_features as ref_features  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import srm0_cases as SC  # noqa: E402


def hook_layer(layer, rec):
    """Record, per forward(): the draws (replayed from the state in front of the call) and s_prob."""
    orig = layer.forward

    def forward(x):
        before = torch.get_rng_state()
        orig(x)
        after = torch.get_rng_state()
        torch.set_rng_state(before)
        u = torch.rand_like(layer.s_prob)
        assert torch.equal(torch.get_rng_state(), after), "forward() drew something besides rand_like(s_prob)"
        assert torch.equal(u < layer.s_prob, layer.s), "the replayed draws do not give the layer's spikes"
        rec["u"].append(u.numpy().astype(np.float32).copy())
        rec["p"].append(layer.s_prob.numpy().astype(np.float32).copy())

    layer.forward = forward


def hook_rule(conn, rec):
    orig = conn.update

    def update(**kwargs):
        rec["x"].append(conn.source.x.numpy().astype(np.float32).reshape(-1).copy())
        orig(**kwargs)

    conn.update = update


def main(only):
    torch.set_num_threads(1)
    ns = SC.ns_from(ref_nodes, ref_topology, ref_features, ref_learning, Network)
    problems = []
    for name, c in SC.CASES.items():
        if only and name not in only:
            continue
        net = SC.build(ns, name)
        layers = SC.srm0_layers(name)
        recs = {L: {"u": [], "p": []} for L in layers}
        for L in layers:
            hook_layer(net.layers[L], recs[L])
        rule_rec = {"x": []}
        if c.get("rule"):
            hook_rule(net.connections[("X", "Y")], rule_rec)
            w0 = SC.weights(net).detach().numpy().copy()
        snaps = SC.run_case(net, name, Monitor)
        T, B = c["T"], c["B"]
        out = {"seed": np.array(c["seed"])}
        for L in layers:                                 # the decays the reference's compute_decays() made on this machine
            out[f"{L}_decay"] = np.asarray(net.layers[L].decay.numpy(), np.float32).copy()
            out[f"{L}_trace_decay"] = np.asarray(net.layers[L].trace_decay.numpy(), np.float32).copy()
        margin, spikes, cells, bad = np.inf, 0, 0, []
        for r, s in enumerate(snaps):
            out[f"r{r}_rng0"], out[f"r{r}_rng1"] = s["rng0"], s["rng1"]
            for L in layers:
                u = np.stack(recs[L]["u"][r * T:(r + 1) * T]).reshape(T, B, -1)
                p = np.stack(recs[L]["p"][r * T:(r + 1) * T]).reshape(T, B, -1)
                assert np.array_equal((u < p).astype(np.uint8), s[L + "_raster"])
                margin = min(margin, float(np.abs(u.astype(np.float64) - p.astype(np.float64)).min()))
                out[f"r{r}_{L}_raster"] = np.packbits(s[L + "_raster"].reshape(-1))
                out[f"r{r}_{L}_vrec"], out[f"r{r}_{L}_prec"], out[f"r{r}_{L}_u"] = s[L + "_vrec"], p, u
                for k in ("v", "rc", "x", "sprob"):
                    out[f"r{r}_{L}_{k}"] = s[f"{L}_{k}"]
                spikes += int(s[L + "_raster"].sum())
                cells += s[L + "_raster"].size
            for k in ("xX", "w", "e"):
                if k in s:
                    out[f"r{r}_{k}"] = s[k]
            if c.get("rule"):
                out[f"r{r}_rx"] = np.stack(rule_rec["x"][r * T:(r + 1) * T])
        out["min_margin"] = np.array(margin)
        rate = spikes / cells
        if not 0.005 < rate < 0.7:
            bad.append(("spike rate", rate))
        if not margin >= SC.MARGIN[bool(c.get("rule"))]:
            bad.append(("least |u - s_prob|", margin))
        if any(not np.isfinite(a).all() for a in out.values() if a.dtype.kind == "f"):
            bad.append(("NaN or infinity", None))
        note = ""
        if c.get("rule"):
            w = snaps[-1]["w"]
            on_bound = float(np.mean((w == c["wmin"]) | (w == c["wmax"]))) if "wmin" in c else 0.0
            moved = float(np.abs(w - w0).max())
            out["w0"] = w0
            if on_bound >= 0.05:
                bad.append(("weights on a bound", on_bound))
            if not moved > 1e-2:
                bad.append(("largest weight movement", moved))
            note = f", on a bound {on_bound:.3f}, largest movement {moved:.3f}"
        if bad:
            problems.append((name, bad))
            print(f"  {name}: NOT written: {bad}")
            continue
        path = os.path.join(HERE, f"srm0_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"  {name}: rate {rate:.3f}, least margin {margin:.3g}{note}, {os.path.getsize(path)} bytes")
    assert not problems, problems


if __name__ == "__main__":
    main(set(sys.argv[1:]))
