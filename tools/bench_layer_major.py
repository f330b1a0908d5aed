#!/usr/bin/env python3
"""Timesteps/s of converted networks on the MI355X with and without the layer-major plan (Network.layer_major), T = 100:

  * cnn: tools/bench_conv_wide.py's converted CNN with its two MaxPool2d children replaced by AvgPool2d(2) -- a MaxPool2dConnection
    feeds a PassThroughNodes layer, which the layer-major plan does not take (the run would be the generic plan on both arms); the
    average-pooled sibling is the qualifying graph of the same shapes: Conv 3-32 / pool / Conv 32-64 / pool / Conv 64-128 / Linear 8192-10;
  * mlp: tools/bench_analog.py's 784 - 256 - 128 - 10.

    python tools/bench_layer_major.py [--time 100] [--runs 10] [--reps 5] [--batch 1 16] [--tree DIR] [--dense-route2]
    python tools/bench_layer_major.py --kernel [--only conv|dense]

Per network, batch size and input kind (Bernoulli spike bytes at 10 %, or the real-valued sample repeated): one untimed run per arm,
then `reps` windows of `runs` network.run(time) + reset_state_variables() per arm, the arms alternating window by window, timed end to
end with the device synchronised.  One JSON line per point: the median window with [min, max] per arm, and each arm's last_plan.
--tree DIR imports the package from another checkout (the parent commit, built there): that tree has no layer_major, so it reports the
generic arm only -- the figure this commit's layer-major arm is compared against, taken in the same session.
--kernel: per convolution of the CNN, one ops.run_conv2d_sif launch over T steps against T x (ops.prop_conv2d_mfma + ops.sif_step),
microseconds per layer-run between device events, and whether the bank stayed resident; per dense layer (784-256, 256-128, 128-10,
8192-10, at 10 % and 50 % density), one ops.run_dense_sif launch against the calls of the plan's route 2.
--dense-route2: on spike input a third arm, the layer-major plan with its dense layers forced to route 2 (the plan as it was before
snn_run_dense_sif_f32), alternating with the others."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CNN_SHAPE = (3, 32, 32)
CNN_BANDS = [(-14, 18), (-8, 8), (-4, 4), (-8, 8), (-2, 2), (-8, 8), (-1, 1), (-8, 8)]      # as bench_conv_wide.py, in 1/64
LAYERS = [(3, 32, 32, 32), (32, 64, 16, 16), (64, 128, 8, 8)]


def model(kind):
    if kind == "mlp":
        torch.manual_seed(0)
        return nn.Sequential(nn.Linear(784, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(), nn.Linear(128, 10)), (784,)
    ann = nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), nn.ReLU(), nn.AvgPool2d(2), nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(), nn.AvgPool2d(2),
                        nn.Conv2d(64, 128, 3, padding=1), nn.ReLU(), nn.Linear(8192, 10))
    rng = np.random.default_rng(0)
    with torch.no_grad():
        for p, (lo, hi) in zip(ann.parameters(), CNN_BANDS):
            p.copy_(torch.from_numpy((rng.integers(lo, hi + 1, size=tuple(p.shape)) / 64.0).astype(np.float32)))
    return ann, CNN_SHAPE


def network(kind, B, layer_major):
    from bindsnet_amd.conversion import ann_to_snn
    ann, shape = model(kind)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        net = ann_to_snn(ann, shape)
    if layer_major:
        net.layer_major = True
    net.batch_size = B
    for l in net.layers.values():
        l.set_batch_size(B)
    return net.to(DEV)


def window(net, x, T, runs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        net.run({"Input": x}, time=T)
        net.reset_state_variables()
    torch.cuda.synchronize()
    return runs * T / (time.perf_counter() - t0)


_fuse_dense = None


def force_dense_route2(on):
    """The --dense-route2 arm: the plan's gate for dense layers answers no, so they run as before snn_run_dense_sif_f32 existed (the
    operator per time chunk into the currents scratch, then snn_sif_scan).  A switch of this tool, not of the library."""
    global _fuse_dense
    from bindsnet_amd.network import layer_major as lm
    if not hasattr(lm, "_fuse_dense"):
        return
    _fuse_dense = _fuse_dense or lm._fuse_dense
    lm._fuse_dense = (lambda *shape: False) if on else _fuse_dense


def end_to_end(a, has_plan):
    for kind in ("cnn", "mlp"):
        shape = model(kind)[1]
        for B in a.batch:
            for analog in (False, True):
                g = torch.Generator().manual_seed(B)
                x = torch.rand(1, B, *shape, generator=g).expand(a.time, B, *shape).contiguous() if analog \
                    else (torch.rand(a.time, B, *shape, generator=g) < 0.1).to(torch.uint8)
                x = x.to(DEV)
                arms = {"generic": network(kind, B, False)}
                if has_plan:
                    arms["layer_major"] = network(kind, B, True)
                if has_plan and a.dense_route2 and not analog:
                    arms["layer_major_dense_route2"] = network(kind, B, True)
                for name, net in arms.items():
                    force_dense_route2(name.endswith("route2"))
                    window(net, x, a.time, 1)                      # untimed
                rates = {name: [] for name in arms}
                for _ in range(a.reps):
                    for name, net in arms.items():
                        force_dense_route2(name.endswith("route2"))
                        rates[name].append(window(net, x, a.time, a.runs))
                force_dense_route2(False)
                line = {"net": kind, "B": B, "T": a.time, "input": "analog" if analog else "spikes", "runs_per_window": a.runs, "windows": a.reps,
                        "tree": a.tree or "."}
                for name, net in arms.items():
                    line[name + "_timesteps_per_s"] = round(statistics.median(rates[name]), 1)
                    line[name + "_min_max"] = [round(min(rates[name]), 1), round(max(rates[name]), 1)]
                    line[name + "_windows"] = [round(r, 1) for r in rates[name]]
                    line[name + "_plan"] = net.last_plan
                print(json.dumps(line), flush=True)


def kernel(a):
    from bindsnet_amd import ops
    from bindsnet_amd._lib import LifParams
    T = a.time
    p = LifParams(thresh=1.0, dt=1.0)
    for cin, cout, h, w in LAYERS:
        W, bias = torch.randn(cout, cin, 3, 3, device=DEV) * 0.1, torch.randn(cout, device=DEV) * 0.1
        for B in a.batch:
            s_train = (torch.rand(T, B, cin, h, w, device=DEV) < 0.1).to(torch.uint8)
            s0 = torch.zeros(B, cin, h, w, dtype=torch.uint8, device=DEV)
            train = torch.empty(T, B, cout, h, w, dtype=torch.uint8, device=DEV)
            v, rc, s = torch.zeros(B, cout, h, w, device=DEV), torch.zeros(B, cout, h, w, device=DEV), torch.zeros(B, cout, h, w, dtype=torch.uint8, device=DEV)
            cur = torch.empty(B, cout, h, w, device=DEV)

            def one_launch():
                ops.run_conv2d_sif(W, bias, s0, s_train, train, v, rc, s, p, stride=1, pad=1)

            def per_step():
                for t in range(T):
                    ops.prop_conv2d_mfma(W, s0 if t == 0 else s_train[t - 1], cur, bias=bias, stride=1, pad=1)
                    ops.sif_step(v, rc, s, None, cur, p, raster_s=train[t])
            us = {"run_conv2d_sif": [], "T x (prop_conv2d_mfma + sif_step)": []}
            for f in (one_launch, per_step):
                f()
            for _ in range(a.reps):
                for name, f in zip(us, (one_launch, per_step)):
                    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for _ in range(a.runs):
                        f()
                    end.record()
                    torch.cuda.synchronize()
                    us[name].append(1000.0 * start.elapsed_time(end) / a.runs)
            print(json.dumps({"Cin": cin, "Cout": cout, "image": [h, w], "B": B, "T": T, "windows": a.reps, "runs_per_window": a.runs,
                              "bank": {1: "resident", 2: "streams"}[ops.run_conv2d_sif_takes(T, B, cin, h, w, cout, 3, 3, 1, 1)],
                              **{name + " us": [round(statistics.median(v_), 1), [round(min(v_), 1), round(max(v_), 1)]] for name, v_ in us.items()}}),
                  flush=True)


DENSE = [(784, 256), (256, 128), (128, 10), (8192, 10)]


def kernel_dense(a):
    """Per dense layer: one ops.run_dense_sif launch over T steps against route 2's calls (prop_dense_auto of the start frame, of the
    other T - 1 frames as (T - 1) x B samples, then sif_scan), microseconds per layer-run between device events."""
    from bindsnet_amd import ops
    from bindsnet_amd._lib import LifParams
    T = a.time
    p = LifParams(thresh=1.0, dt=1.0)
    for nin, n in DENSE:
        W, bias = torch.randn(nin, n, device=DEV) * (2.0 / nin ** 0.5), torch.randn(n, device=DEV) * 0.1
        for B in a.batch:
            for density in (0.1, 0.5):
                s_train = (torch.rand(T, B, nin, device=DEV) < density).to(torch.uint8)
                s0 = torch.zeros(B, nin, dtype=torch.uint8, device=DEV)
                train, cur = torch.empty(T, B, n, dtype=torch.uint8, device=DEV), torch.empty(T, B, n, device=DEV)
                v, rc, s = torch.zeros(B, n, device=DEV), torch.zeros(B, n, device=DEV), torch.zeros(B, n, dtype=torch.uint8, device=DEV)
                flags = torch.zeros(((T - 1) * B + 15) // 16, dtype=torch.int32, device=DEV)

                def one_launch():
                    ops.run_dense_sif(W, bias, s0, s_train, train, v, rc, s, p)

                def route2():
                    ops.prop_dense_auto(W, s0, cur[0], bias=bias, flags=flags)
                    ops.prop_dense_auto(W, s_train[:T - 1].view(-1, nin), cur[1:].view(-1, n), bias=bias, flags=flags)
                    ops.sif_scan(v, rc, s, None, cur, train, p)
                us = {"run_dense_sif": [], "route 2 (2 x prop_dense_auto + sif_scan)": []}
                for f in (one_launch, route2):
                    f()
                for _ in range(a.reps):
                    for name, f in zip(us, (one_launch, route2)):
                        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        start.record()
                        for _ in range(a.runs):
                            f()
                        end.record()
                        torch.cuda.synchronize()
                        us[name].append(1000.0 * start.elapsed_time(end) / a.runs)
                print(json.dumps({"Nin": nin, "N": n, "B": B, "T": T, "density": density, "windows": a.reps, "runs_per_window": a.runs,
                                  "panel": {1: "resident", 2: "streams"}[ops.run_dense_sif_takes(T, B, nin, n)],
                                  **{name + " us": [round(statistics.median(v_), 1), [round(min(v_), 1), round(max(v_), 1)]] for name, v_ in us.items()}}),
                      flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=100)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--tree", default=None, help="another checkout of this project, built, to import bindsnet_amd from")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--dense-route2", action="store_true", help="a third arm: the layer-major plan with its dense layers forced to route 2")
    ap.add_argument("--only", choices=("conv", "dense"), default=None, help="with --kernel: one family of layers only")
    a = ap.parse_args()
    if a.reps < 3:
        raise SystemExit("bench_layer_major.py reports a spread: at least 3 windows")
    if not torch.cuda.is_available():
        raise SystemExit("bench_layer_major.py measures on the MI355X: no GPU here")
    root = os.path.abspath(a.tree) if a.tree is not None else ROOT
    if not os.path.isfile(os.path.join(root, "bindsnet_amd", "__init__.py")):
        raise SystemExit(f"--tree {a.tree}: no bindsnet_amd package there")
    sys.path[:0] = [root]
    from bindsnet_amd.network import Network
    if not a.kernel:
        return end_to_end(a, hasattr(Network, "layer_major"))
    if a.only != "dense":
        kernel(a)
    if a.only != "conv":
        kernel_dense(a)


if __name__ == "__main__":
    main()
