#!/usr/bin/env python3
"""Steps per second of a converted network (information only; profiles/NOTES_conversion.md): the 784-256-128-10 MLP of the
reference's test/conversion through ann_to_snn, Bernoulli input, batch B, T steps per run -- on the device (generic plan) and on
the package's host path, on the same machine.

Timed with the host clock around `repeats` runs of Network.run, each followed by reset_state_variables(), ending in
torch.cuda.synchronize() for the device; two untimed runs first.  Prints one JSON line per path.  Needs a GPU for the device figure:
without one it fails rather than reporting a host number in its place."""
import argparse
import json
import os
import sys
import time
import warnings

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def network(device):
    from bindsnet_amd.conversion import ann_to_snn
    torch.manual_seed(0)
    ann = nn.Sequential(nn.Linear(784, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(), nn.Linear(128, 10))
    with torch.no_grad():
        for p in ann.parameters():
            p *= 3.0                      # (the default initialisation leaves the last layers silent within 100 steps)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        net = ann_to_snn(ann, (784,))
    return net.to(device)


def measure(device, B, T, repeats):
    net = network(device)
    x = (torch.rand(T, B, 784, generator=torch.Generator().manual_seed(1)) < 0.3).to(torch.uint8).to(device)
    sync = torch.cuda.synchronize if device != "cpu" else (lambda: None)
    for _ in range(2):
        net.run({"Input": x}, time=T)
        net.reset_state_variables()
    sync()
    t0 = time.perf_counter()
    for _ in range(repeats):
        net.run({"Input": x}, time=T)
        net.reset_state_variables()
    sync()
    dt = time.perf_counter() - t0
    net.run({"Input": x}, time=T)
    sync()
    readout = list(net.layers.values())[-1].summed
    return {"device": device, "plan": net.last_plan, "B": B, "T": T, "repeats": repeats, "seconds": round(dt, 4),
            "steps_per_second": round(repeats * T / dt, 1), "sample_steps_per_second": round(repeats * T * B / dt, 1),
            "readout_abs_sum": float(readout.abs().sum())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=500)
    ap.add_argument("--host-repeats", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conversion: no GPU: the device figure cannot be measured here")
    print(json.dumps(measure("cuda:0", a.batch, a.steps, a.repeats)))
    print(json.dumps(measure("cpu", a.batch, a.steps, a.host_repeats)))
