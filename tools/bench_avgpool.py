#!/usr/bin/env python3
"""AvgPool2dConnection on the MI355X: the cost of one pooling call, the crossover between the kernel's two bodies, and a converted CNN
with BatchNorm and average pooling end to end.

    python tools/bench_avgpool.py [--ops] [--crossover] [--net] [--time 100] [--batch 1 16] [--calls 2000] [--runs 20] [--host-runs 2]

Without a selection all three parts run.  Every figure is the median of 5 timed windows with [min - max]; every window follows an
untimed warm-up of the same work and ends in a device synchronise.  One JSON line per point.

--ops        us per call of ops.prop_avgpool's kernel (kernel 2, stride 2) against ops.prop_pool's (MaxPool2dConnection, same window,
             decay 1) on the same planes: (32, 32, 32) and (64, 16, 16) at B = 1 and 16, spikes at 30 %.  `calls` calls per window, made
             straight at the library's entry points with arguments built once, as the generic plan makes them: a call that takes less
             than the enqueue shows the enqueue.
--crossover  us per call of the per-thread and of the per-wave body (snn_set_avgpool_body 1 / 2) for whole-plane windows -- kernel =
             stride = the plane, 64 channels, B = 1 and 16 -- of 4 .. 1024 taps, and for 2x2 .. 8x8 windows tiling a (64, 32, 32) plane
             group: where the per-wave body starts to win is SNN_AVGPOOL_COOP_TAPS (include/snnhip.h).
--net        timesteps/s of a (3, 32, 32) Conv32-BN-ReLU-AvgPool2-Conv64-BN-ReLU-AdaptiveAvgPool(1)-Flatten-Linear10 model converted by
             ann_to_snn (data-based normalisation on 64 random images) at T = `time`, B = 1 and 16, on the device (generic plan) and on the
             host path: `runs` / `host-runs` network.run(time) calls per window, each followed by reset_state_variables(); the real-valued
             image is repeated over time, as converted networks are driven.  The readout `summed` of both sides is compared (largest
             difference over its largest magnitude: the convolutions sum in different orders)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
DEV = "cuda:0"
WINDOWS = 5


def windows(fn, n, sync):
    """us per call of fn over WINDOWS windows of n calls each: (median, min, max)."""
    fn()
    sync()
    per = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        per.append(1e6 * (time.perf_counter() - t0) / n)
    return round(statistics.median(per), 2), round(min(per), 2), round(max(per), 2)


def spread(triple):
    return {"median": triple[0], "min": triple[1], "max": triple[2]}


def avgpool_call(s, out, k):
    """One snn_prop_avgpool2d_f32 call (kernel = stride = k) with its arguments built once: what ops.prop_avgpool hands the library, without the
    wrapper's checks, so that the host's share of a call is the enqueue alone -- as in the generic plan, which calls it from C++."""
    from bindsnet_amd import _lib, ops
    arrays, pooled = ops.avgpool_geometry(s.shape[2:], k, k)
    assert tuple(out.shape[2:]) == pooled
    fn, args = _lib.lib().snn_prop_avgpool2d_f32, (s.data_ptr(), out.data_ptr(), s.shape[0], s.shape[1], *arrays, 0, 1, 0, 0, ops._stream())
    return lambda: fn(*args)


def maxpool_call(fr, s, out, k):
    from bindsnet_amd import _lib, ops
    arrays, pooled = ops.pool_geometry(s.shape[2:], k, k, 0, 1)
    assert tuple(out.shape[2:]) == pooled
    fn, args = _lib.lib().snn_prop_pool_f32, (fr.data_ptr(), s.data_ptr(), out.data_ptr(), s.shape[0], s.shape[1], *arrays, 1.0, 0, ops._stream())
    return lambda: fn(*args)


def ops_part(a):
    for (C, H, W) in ((32, 32, 32), (64, 16, 16)):
        for B in a.batch:
            g = torch.Generator().manual_seed(B + C)
            s = (torch.rand(B, C, H, W, generator=g) < 0.3).to(torch.uint8).to(DEV)
            out, fr = torch.zeros(B, C, H // 2, W // 2, device=DEV), torch.zeros(B, C, H, W, device=DEV)
            avg = windows(avgpool_call(s, out, (2, 2)), a.calls, torch.cuda.synchronize)
            mx = windows(maxpool_call(fr, s, out, (2, 2)), a.calls, torch.cuda.synchronize)
            print(json.dumps({"part": "ops", "plane": [C, H, W], "B": B, "calls_per_window": a.calls, "prop_avgpool_us": spread(avg),
                              "prop_pool_us": spread(mx)}), flush=True)


def crossover_part(a):
    from bindsnet_amd import _lib
    L = _lib.lib()
    points = [("whole-plane", 64, (k0, k1), (k0, k1)) for k0, k1 in ((2, 2), (2, 4), (4, 4), (4, 8), (8, 8), (8, 16), (16, 16), (32, 32))]
    points += [("tiled", 64, (32, 32), (k, k)) for k in (2, 4, 8)]
    try:
        for what, C, plane, k in points:
            for B in a.batch:
                g = torch.Generator().manual_seed(B + k[0] * k[1])
                s = (torch.rand(B, C, *plane, generator=g) < 0.3).to(torch.uint8).to(DEV)
                out = torch.zeros(B, C, plane[0] // k[0], plane[1] // k[1], device=DEV)
                line = {"part": "crossover", "case": what, "plane": [C, *plane], "kernel": list(k), "taps": k[0] * k[1], "B": B, "outputs": out.numel(),
                        "calls_per_window": a.calls}
                for body, name in ((1, "per_thread_us"), (2, "per_wave_us")):
                    L.snn_set_avgpool_body(body)
                    line[name] = spread(windows(avgpool_call(s, out, k), a.calls, torch.cuda.synchronize))
                line["per_wave_over_per_thread"] = round(line["per_wave_us"]["median"] / line["per_thread_us"]["median"], 3)
                print(json.dumps(line), flush=True)
    finally:
        L.snn_set_avgpool_body(0)


def model():
    import torch.nn as nn
    torch.manual_seed(0)
    ann = nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), nn.BatchNorm2d(32), nn.ReLU(), nn.AvgPool2d(2), nn.Conv2d(32, 64, 3, padding=1), nn.BatchNorm2d(64),
                        nn.ReLU(), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(64, 10))
    with torch.no_grad():
        for m in ann:
            if isinstance(m, nn.BatchNorm2d):                      # statistics as a trained model has them, not the identity of a fresh one
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    return ann.eval()


def net_part(a):
    import warnings
    from bindsnet_amd.conversion import ann_to_snn
    ann = model()
    data = torch.rand(64, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    for B in a.batch:
        image = torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(10 + B))
        x = image.repeat(a.time, 1, 1, 1, 1)
        line = {"part": "net", "graph": "ann_to_snn(Conv32-BN-ReLU-AvgPool2-Conv64-BN-ReLU-AdaptiveAvgPool(1)-Flatten-Linear10), input (3, 32, 32), analog",
                "B": B, "T": a.time}
        summed = {}
        for side in ("device", "host"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                net = ann_to_snn(ann, (3, 32, 32), data=data)
            xs, sync, runs = (x.to(DEV), torch.cuda.synchronize, a.runs) if side == "device" else (x, lambda: None, a.host_runs)
            if side == "device":
                net = net.to(DEV)
            net.run({"Input": xs.clone()}, time=a.time)
            summed[side] = net.layers["10"].summed.detach().cpu().clone()
            net.reset_state_variables()

            def once():
                net.run({"Input": xs.clone()}, time=a.time)
                net.reset_state_variables()
            us = windows(once, runs, sync)
            line[side + "_timesteps_per_s"] = {"median": round(1e6 * a.time / us[0], 1), "min": round(1e6 * a.time / us[2], 1), "max": round(1e6 * a.time / us[1], 1)}
            line[side + "_runs_per_window"], line[side + "_plan"] = runs, net.last_plan
        scale = float(summed["host"].abs().max())
        line["summed_max_abs"] = round(scale, 4)
        line["summed_device_minus_host_over_max"] = float((summed["device"] - summed["host"]).abs().max()) / scale if scale else None
        line["device_over_host"] = round(line["device_timesteps_per_s"]["median"] / line["host_timesteps_per_s"]["median"], 2)
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    for part in ("ops", "crossover", "net"):
        ap.add_argument("--" + part, action="store_true")
    ap.add_argument("--time", type=int, default=100)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_avgpool.py measures on the MI355X: no GPU here")
    every = not (a.ops or a.crossover or a.net)
    if a.ops or every:
        ops_part(a)
    if a.crossover or every:
        crossover_part(a)
    if a.net or every:
        net_part(a)


if __name__ == "__main__":
    main()
