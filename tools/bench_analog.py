#!/usr/bin/env python3
"""Timesteps/s of converted networks driven by the real-valued sample itself (encoding.repeat: the float32 image at every step), on the
MI355X and on the package's host path, same commit, same machine; the same networks on the device with a uint8 Poisson train of
matching mean rate; and the ordered dense kernel alone against torch.mm.

    python tools/bench_analog.py [--time 100] [--runs 20] [--host-runs 2] [--reps 5] [--batch 1 16] [--calls]

Networks: a converted MLP 784-256-128-10 and the converted CNN of tools/bench_conv_wide.py ((3, 32, 32) input).  The image is zero in
about 60 % of its pixels (MNIST-like), uniform in (0, 1) elsewhere.  Per network and batch size one JSON line: per leg one untimed
run, then `reps` windows of `runs` network.run(time) calls, each followed by reset_state_variables(), timed end to end (the device
synchronised); the median window's timesteps/s with the least and the largest.  Legs: `analog` (float32 input on the device),
`poisson` (uint8 Bernoulli train whose rate per pixel is the image's value, on the device), `host` (the analog input on the host path).

--calls: ops.prop_dense_real against torch.mm at the MLP's [B, Nin] x [Nin, N] shapes, and ops.prop_conv2d_real at the CNN's first
layer: 3 untimed calls, then `reps` windows of 100 calls between device events; the median microseconds per call with the spread."""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
DEV = "cuda:0"
MLP = (784, 256, 128, 10)


def mlp_model():
    ann = nn.Sequential(nn.Linear(784, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(), nn.Linear(128, 10))
    rng = np.random.default_rng(0)
    with torch.no_grad():
        for p in ann.parameters():             # (small weights: hidden rates of a few per cent at an MNIST-like input)
            p.copy_(torch.from_numpy(((rng.random(tuple(p.shape)) * 2 - 0.9) * (0.08 if p.dim() > 1 else 0.05)).astype(np.float32)))
    return ann


def network(kind, B):
    import bench_conv_wide
    from bindsnet_amd.conversion import ann_to_snn
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        net = ann_to_snn(mlp_model(), (784,)) if kind == "mlp" else ann_to_snn(bench_conv_wide.model(), bench_conv_wide.SHAPE)
    net.batch_size = B
    for l in net.layers.values():
        l.set_batch_size(B)
    for c in net.connections.values():
        c.reset_state_variables()
    return net


def image(kind, B):
    shape = (784,) if kind == "mlp" else (3, 32, 32)
    g = torch.Generator().manual_seed(B)
    return torch.rand(B, *shape, generator=g) * (torch.rand(B, *shape, generator=g) < 0.4)


def timed(net, x, T, runs, reps, sync):
    from bindsnet_amd.network.monitors import Monitor
    mons = {l: Monitor(layer, ["s"], time=T) for l, layer in net.layers.items() if hasattr(layer, "refrac_count")}
    for l, m in mons.items():
        net.add_monitor(m, l)
    net.run({"Input": x.clone()}, time=T)                      # untimed; the spikes per neuron-step are taken here
    spikes = {l: round(float(m.get("s").float().mean()), 4) for l, m in mons.items()}
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
    return rates, spikes


def end_to_end(a):
    for kind in ("mlp", "cnn"):
        for B in a.batch:
            img = image(kind, B)
            analog = img.unsqueeze(0).repeat(a.time, *([1] * img.dim())).contiguous()
            poisson = (torch.rand(a.time, *img.shape, generator=torch.Generator().manual_seed(100 + B)) < img).to(torch.uint8)
            line = {"graph": "ann_to_snn MLP 784-256-128-10" if kind == "mlp" else "ann_to_snn CNN of bench_conv_wide.py, input 3x32x32", "B": B, "T": a.time,
                    "input_mean": round(float(img.mean()), 4), "poisson_rate": round(float(poisson.float().mean()), 4)}
            for leg, x, dev in (("analog", analog, True), ("poisson", poisson, True), ("host", analog, False)):
                net = network(kind, B)
                if dev:
                    net = net.to(DEV)
                runs = a.runs if dev else a.host_runs
                rates, line[leg + "_spikes_per_neuron_step"] = timed(net, x.to(DEV) if dev else x, a.time, runs, a.reps,
                                                                     torch.cuda.synchronize if dev else (lambda: None))
                line[leg + "_timesteps_per_s"] = round(statistics.median(rates), 1)
                line[leg + "_timesteps_per_s_min_max"] = [round(min(rates), 1), round(max(rates), 1)]
                line[leg + "_runs_per_window"], line[leg + "_plan"] = runs, net.last_plan
            line["windows"] = a.reps
            line["analog_over_poisson"] = round(line["analog_timesteps_per_s"] / line["poisson_timesteps_per_s"], 2)
            line["analog_over_host"] = round(line["analog_timesteps_per_s"] / line["host_timesteps_per_s"], 2)
            print(json.dumps(line), flush=True)


def _window(fn, reps, n=100):
    for _ in range(3):
        fn()
    us = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            fn()
        end.record()
        torch.cuda.synchronize()
        us.append(1000.0 * start.elapsed_time(end) / n)
    return round(statistics.median(us), 2), [round(min(us), 2), round(max(us), 2)]


def calls(a):
    from bindsnet_amd import ops
    for B in a.batch:
        for nin, n in zip(MLP[:-1], MLP[1:]):
            for density in (0.4, 1.0):                             # the image's share of non-zero pixels; a dense input
                W, bias = torch.randn(nin, n, device=DEV), torch.randn(n, device=DEV)
                x = (torch.rand(B, nin, device=DEV) * (torch.rand(B, nin, device=DEV) < density)).contiguous()
                out, ref = torch.empty(B, n, device=DEV), torch.empty(B, n, device=DEV)
                real = _window(lambda: ops.prop_dense_real(W, x, out, bias=bias), a.reps)
                mm = _window(lambda: torch.addmm(bias, x, W, out=ref), a.reps)
                print(json.dumps({"op": "prop_dense_real", "B": B, "Nin": nin, "N": n, "nonzero": density, "calls_per_window": 100, "windows": a.reps,
                                  "us_per_call": real[0], "us_per_call_min_max": real[1], "torch_addmm_us_per_call": mm[0],
                                  "torch_addmm_us_per_call_min_max": mm[1], "real_over_mm": round(real[0] / mm[0], 2),
                                  "max_abs_diff_vs_mm": float((out - ref).abs().max())}), flush=True)
        W, bias = torch.randn(32, 3, 3, 3, device=DEV), torch.randn(32, device=DEV)
        x = (torch.rand(B, 3, 32, 32, device=DEV) * (torch.rand(B, 3, 32, 32, device=DEV) < 0.4)).contiguous()
        out = torch.empty(B, 32, 32, 32, device=DEV)
        real = _window(lambda: ops.prop_conv2d_real(W, x, out, bias=bias, stride=1, pad=1), a.reps)
        s = (x != 0).to(torch.uint8)
        byte = _window(lambda: ops.prop_conv2d(W, s, out, bias=bias, stride=1, pad=1), a.reps)
        print(json.dumps({"op": "prop_conv2d_real", "Cin": 3, "Cout": 32, "image": [32, 32], "kernel": [3, 3], "pad": 1, "B": B, "nonzero": 0.4,
                          "calls_per_window": 100, "windows": a.reps, "us_per_call": real[0], "us_per_call_min_max": real[1],
                          "prop_conv2d_same_density_us_per_call": byte[0], "prop_conv2d_same_density_us_per_call_min_max": byte[1]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=100)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    a = ap.parse_args()
    if a.reps < 3:
        raise SystemExit("bench_analog.py reports a spread: at least 3 windows")
    if not torch.cuda.is_available():
        raise SystemExit("bench_analog.py measures on the MI355X: no GPU here")
    return calls(a) if a.calls else end_to_end(a)


if __name__ == "__main__":
    main()
