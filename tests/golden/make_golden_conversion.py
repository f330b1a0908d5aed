#!/usr/bin/env python3
"""Fixtures of bindsnet.conversion: the UNMODIFIED reference's CPU path (build container only) over the cases of
tests/conversion_cases.py.  Writes tests/golden/conversion_<case>.npz, conversion_norm.npz and conversion_raises.json.

One thing the reference cannot do as it stands: PermuteConnection and ConstantPad2dConnection do not define the two abstract
methods of AbstractConnection (`update`, `reset_state_variables`), so constructing either raises TypeError -- and with it every
ann_to_snn over a Permute or ConstantPad2d child.  conversion_raises.json records that ("reference").  To have something to pin
their compute() against, the generator derives from each class a subclass that adds nothing but the two missing methods (the
bodies the reference's own Connection uses) and an empty normalize(), which Network.run calls on every connection, and puts those in the places the reference looks its classes up; compute(), the helper
and everything else stay the reference's text.  What the calls do then is recorded as "concrete".

Per case and input: the bit-packed rasters of every non-Input layer, final v, refrac_count, x and summed of the spiking layers, the
pooling firing_rates.  A fixture is written only if
  * every non-Input layer's spike rate lies strictly between 0 and 1 (step cases: step 0 is all spikes, step 1 none);
  * dyadic family: the reference at 1 thread equals the reference at 8 threads bit for bit in every field (the sums are exact);
  * float family: the stated order (conversion_cases.stated_run) reproduces the reference's rasters, refrac_count and traces bit for
    bit, and every |v - thresh| met before a reset is at least MARGIN x v_spread, v_spread = max |reference - stated| over the
    per-step v; seeds are searched until that holds, and the seed, v_spread and summed_spread are stored.

    python tests/golden/make_golden_conversion.py [case ...]"""
import json
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
from bindsnet.conversion import conversion as ref_conversion_module  # noqa: E402
from bindsnet.network import nodes as ref_nodes, topology as ref_topology  # noqa: E402
from bindsnet.network.monitors import Monitor  # noqa: E402
from bindsnet.network.network import Network  # noqa: E402
import conversion_cases as CC  # noqa: E402


def concrete(cls):
    """`cls` with the two abstract methods it lacks, as the reference's Connection has them."""
    def update(self, **kwargs):
        super(sub, self).update(**kwargs)

    def reset_state_variables(self):
        super(sub, self).reset_state_variables()

    def normalize(self):
        """Network.run calls it on every connection behind the loop; there are no weights."""

    sub = type(cls.__name__, (cls,), {"update": update, "reset_state_variables": reset_state_variables, "normalize": normalize})
    return sub


def namespaces():
    plain = CC.ns_from(ref_nodes, ref_topology, Network, Monitor, ref_conversion)
    shim = types.SimpleNamespace(**vars(ref_conversion))
    shim.PermuteConnection, shim.ConstantPad2dConnection = concrete(ref_conversion.PermuteConnection), concrete(ref_conversion.ConstantPad2dConnection)
    return plain, CC.ns_from(ref_nodes, ref_topology, Network, Monitor, shim), shim


class patched:
    """The helper of ann_to_snn finds the two classes as globals of its module: while a case runs they are the concrete ones."""

    def __init__(self, shim):
        self.shim = shim

    def __enter__(self):
        self.kept = (ref_conversion_module.PermuteConnection, ref_conversion_module.ConstantPad2dConnection)
        ref_conversion_module.PermuteConnection, ref_conversion_module.ConstantPad2dConnection = self.shim.PermuteConnection, self.shim.ConstantPad2dConnection

    def __exit__(self, *exc):
        ref_conversion_module.PermuteConnection, ref_conversion_module.ConstantPad2dConnection = self.kept


def reference(ns, name, threads, seed=None):
    torch.set_num_threads(threads)
    try:
        net = CC.build(ns, name, seed=seed, eval_mode=True)
        params = CC.net_params(net) if name in CC.NETS else None
        return CC.run_case(ns, net, name), params, net
    finally:
        torch.set_num_threads(1)


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def rates_ok(name, snaps, bad):
    for r, s in enumerate(snaps):
        for k, v in s.items():
            if k.endswith("_raster"):
                rate = float(v.mean())
                if not 0.0 < rate < 1.0:
                    bad.append((f"input {r} {k} rate", rate))
        if name in CC.STEP and not (s["Y_raster"][0].all() and not s["Y_raster"][1].any()):
            bad.append((f"input {r}: step 0 must be all spikes, step 1 none", None))


def main(only):
    plain, ns, shim = namespaces()
    problems = []
    with patched(shim):
        for name in CC.CASES:
            if only and name not in only:
                continue
            bad, out = [], {}
            float_case = name in CC.FLOAT
            if not float_case:
                snaps, params, net = reference(ns, name, 1)
                snaps8, _, _ = reference(ns, name, 8)
                for r, (a, b) in enumerate(zip(snaps, snaps8)):
                    for k in a:
                        if not same(a[k], b[k]):
                            bad.append((f"input {r} {k}: 1 thread != 8 threads", None))
                stated = CC.stated_run(name)
                for r, (a, b) in enumerate(zip(snaps, stated)):       # (the stated order must give the exact result too: it pins the test's own helper)
                    for k in a:
                        if not same(a[k], np.asarray(b[k], a[k].dtype).reshape(a[k].shape)):
                            bad.append((f"input {r} {k}: stated order != reference", None))
                seed = CC.seed_of(name)
            else:
                for seed in range(CC.seed_of(name), CC.seed_of(name) + 4000, 100):
                    snaps, params, net = reference(ns, name, 1, seed=seed)
                    stated = CC.stated_run(name, params=params if CC.stores_params(name) else None, seed=seed)
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
                    if exact and margin >= CC.MARGIN * v_spread:
                        break
                else:
                    bad.append(("no seed with the margin", None))
                out.update(v_spread=np.array(v_spread), summed_spread=np.array(summed_spread), least_margin=np.array(margin))
                if CC.stores_params(name):
                    for k, a in enumerate(params):
                        out[f"param{k}"] = a
            out["seed"] = np.array(seed)
            rates_ok(name, snaps, bad)
            for r, s in enumerate(snaps):
                for k, v in s.items():
                    if k.endswith("_vrec"):
                        continue                              # (per-step voltages: used for the spread, not stored)
                    out[f"r{r}_{k}"] = np.packbits(v.reshape(-1)) if k.endswith("_raster") else v
            if name in CC.NETS:                               # what ann_to_snn made: keys, shapes, parameters
                out["layers"] = np.array(json.dumps([(k, type(l).__name__, [int(x) for x in l.shape]) for k, l in net.layers.items()]))
                out["connections"] = np.array(json.dumps([(list(k), type(c).__name__) for k, c in net.connections.items()]))
                out["params_sha"] = np.array(json.dumps([CC.sha(a) for a in params]))
            if any(not np.isfinite(a).all() for a in out.values() if a.dtype.kind == "f"):
                bad.append(("NaN or infinity", None))
            if bad:
                problems.append((name, bad))
                print(f"  {name}: NOT written: {bad[:4]}")
                continue
            path = os.path.join(HERE, f"conversion_{name}.npz")
            np.savez_compressed(path, **out)
            rate = np.mean([v.mean() for s in snaps for k, v in s.items() if k.endswith("_raster")])
            print(f"  {name}: mean rate {rate:.3f}, {os.path.getsize(path)} bytes")

        if not only or "norm" in only:
            out = {}
            for kind in ("mlp", "cnn"):
                ann, data, shape = CC.norm_case(kind)
                before = [p.detach().numpy().copy() for p in ann.parameters()]
                got = ref_conversion.data_based_normalization(ann, data)
                assert got is ann
                for k, p in enumerate(ann.parameters()):
                    out[f"{kind}_{k}"] = p.detach().numpy().copy()
                assert any(not np.array_equal(a, out[f"{kind}_{k}"]) for k, a in enumerate(before)), "the normalisation changed nothing"
            np.savez_compressed(os.path.join(HERE, "conversion_norm.npz"), **out)
            print("  norm: written")

    if not only or "raises" in only:
        rec = {}
        for call in CC.CALLS:
            rec[call] = {"reference": CC.outcome(plain, call)}
            with patched(shim):
                rec[call]["concrete"] = CC.outcome(ns, call)
        for cls in ("PermuteConnection", "ConstantPad2dConnection"):
            try:
                getattr(ref_conversion, cls)(ref_nodes.Input(n=4), ref_nodes.Input(n=4), (0, 1))
                rec["construct_" + cls] = {"reference": "ok"}
            except Exception as e:                            # noqa: BLE001
                rec["construct_" + cls] = {"reference": type(e).__name__}
        json.dump(rec, open(os.path.join(HERE, "conversion_raises.json"), "w"), indent=1, sort_keys=True)
        print(json.dumps(rec, indent=1, sort_keys=True))
    assert not problems, problems


if __name__ == "__main__":
    main(set(sys.argv[1:]))
