#!/usr/bin/env python3
"""Timesteps/s of a converted CNN whose convolutions have 3, 32 and 64 input channels -- ann_to_snn of Conv(3 -> 32, 3, p1) - ReLU -
MaxPool(2) - Conv(32 -> 64, 3, p1) - ReLU - MaxPool(2) - Conv(64 -> 128, 3, p1) - ReLU - Linear(8192 -> 10) on a (3, 32, 32) input,
T = 100 -- on the MI355X (generic plan; the second and third convolution run csrc/snn_conv_wide.hip) and on the package's host path,
same commit, same machine; and the time of one snn_prop_conv2d_f32 call at the three layer shapes.

    python tools/bench_conv_wide.py [--time 100] [--runs 20] [--host-runs 2] [--reps 3] [--batch 1 16] [--calls]

End to end, per batch size in {1, 16}: Bernoulli input at 10 %; weights on a 1/64 grid (every sum exact, so the device's rasters must
equal the host path's: reported).  Per side one untimed run, then `reps` windows of `runs` network.run(time) calls, each followed by
reset_state_variables(), timed end to end (the device synchronised).  One JSON line per point: the median window's timesteps/s of
both sides with the least and the largest, the spikes per neuron-step of every spiking layer, whether the rasters agree.

--calls: per layer shape, batch size in {1, 16} and input density in {1 %, 10 %}: 3 untimed calls, then `reps` windows of 50 calls between
device events; the median microseconds per call with the least and the largest."""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
DEV = "cuda:0"
SHAPE = (3, 32, 32)
LAYERS = [(3, 32, 32, 32), (32, 64, 16, 16), (64, 128, 8, 8)]          # Cin, Cout, H, W of the three convolutions (3x3, pad 1)
BANDS = [(-14, 18), (-8, 8), (-4, 4), (-8, 8), (-2, 2), (-8, 8), (-1, 1), (-8, 8)]      # weight and bias of each layer, in 1/64


def model():
    ann = nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(), nn.MaxPool2d(2),
                        nn.Conv2d(64, 128, 3, padding=1), nn.ReLU(), nn.Linear(8192, 10))
    rng = np.random.default_rng(0)
    with torch.no_grad():
        for p, (lo, hi) in zip(ann.parameters(), BANDS):
            p.copy_(torch.from_numpy((rng.integers(lo, hi + 1, size=tuple(p.shape)) / 64.0).astype(np.float32)))
    return ann


def network(B):
    from bindsnet_amd.conversion import ann_to_snn
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        net = ann_to_snn(model(), SHAPE)
    net.batch_size = B
    for l in net.layers.values():
        l.set_batch_size(B)
    for c in net.connections.values():
        c.reset_state_variables()
    return net


def timed(net, x, T, runs, reps, sync):
    from bindsnet_amd.network.monitors import Monitor
    spiking = [l for l, layer in net.layers.items() if hasattr(layer, "refrac_count")]
    mons = {l: Monitor(net.layers[l], ["s"], time=T) for l in spiking}
    for l, m in mons.items():
        net.add_monitor(m, l)
    net.run({"Input": x.clone()}, time=T)                      # untimed; also what the rasters are compared on
    rasters = {l: m.get("s").clone().cpu() for l, m in mons.items()}
    for l in mons:
        del net.monitors[l]
    net.reset_state_variables()
    rates = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        for _ in range(runs):
            net.run({"Input": x.clone()}, time=T)
            net.reset_state_variables()
        sync()
        rates.append(runs * T / (time.perf_counter() - t0))
    return rates, rasters


def end_to_end(a):
    for B in a.batch:
        x = (torch.rand(a.time, B, *SHAPE, generator=torch.Generator().manual_seed(B)) < 0.1).to(torch.uint8)
        line = {"graph": "ann_to_snn: Conv 3-32 / pool / Conv 32-64 / pool / Conv 64-128 / Linear 8192-10, input 3x32x32", "B": B, "T": a.time}
        rasters = {}
        for side in ("device", "host"):
            net = network(B)
            if side == "device":
                net = net.to(DEV)
            runs = a.runs if side == "device" else a.host_runs
            rates, rasters[side] = timed(net, x.to(DEV) if side == "device" else x, a.time, runs, a.reps,
                                         torch.cuda.synchronize if side == "device" else (lambda: None))
            line[side + "_timesteps_per_s"] = round(statistics.median(rates), 1)
            line[side + "_timesteps_per_s_min_max"] = [round(min(rates), 1), round(max(rates), 1)]
            line[side + "_runs_per_window"], line[side + "_windows"], line[side + "_plan"] = runs, a.reps, net.last_plan
        line["spikes_per_neuron_step"] = {l: round(float(r.float().mean()), 4) for l, r in rasters["device"].items()}
        line["rasters_equal_host"] = all(torch.equal(rasters["device"][l], rasters["host"][l]) for l in rasters["device"])
        line["device_over_host"] = round(line["device_timesteps_per_s"] / line["host_timesteps_per_s"], 2)
        print(json.dumps(line), flush=True)


def calls(a):
    from bindsnet_amd import ops
    for cin, cout, h, w in LAYERS:
        W, bias = torch.randn(cout, cin, 3, 3, device=DEV), torch.randn(cout, device=DEV)
        for B in a.batch:
            out = torch.empty(B, cout, h, w, device=DEV)
            for density in (0.01, 0.1):
                s = (torch.rand(B, cin, h, w, device=DEV) < density).to(torch.uint8)
                for _ in range(3):
                    ops.prop_conv2d(W, s, out, bias=bias, stride=1, pad=1)
                us = []
                for _ in range(a.reps):
                    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for _ in range(50):
                        ops.prop_conv2d(W, s, out, bias=bias, stride=1, pad=1)
                    end.record()
                    torch.cuda.synchronize()
                    us.append(1000.0 * start.elapsed_time(end) / 50)
                print(json.dumps({"op": "prop_conv2d", "Cin": cin, "Cout": cout, "image": [h, w], "kernel": [3, 3], "pad": 1, "B": B, "density": density,
                                  "calls_per_window": 50, "windows": a.reps, "us_per_call": round(statistics.median(us), 2),
                                  "us_per_call_min_max": [round(min(us), 2), round(max(us), 2)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=100)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    a = ap.parse_args()
    if a.reps < 3:
        raise SystemExit("bench_conv_wide.py reports a spread: at least 3 windows")
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_wide.py measures on the MI355X: no GPU here")
    return calls(a) if a.calls else end_to_end(a)


if __name__ == "__main__":
    main()
