#!/usr/bin/env python3
"""Timesteps/s of an SRM0 graph: Input 784 (additive traces) -> Connection -> SRM0Nodes 100, T = 250 --

    rmax    with Rmax on the connection, reward 1.0, B = 1 (all the rule allows)
    plain   without a rule, B = 1 and B = 16

each on the MI355X (generic plan: per timestep one propagation launch, one snn_srm0_step launch that draws and updates, one
snn_rmax_step launch with the rule) and on the package's host path (plain PyTorch, network/host_path.py).

    python tools/bench_srm0.py [--time 250] [--windows 5] [--runs 300] [--host-runs 16] [--no-host]

Per row: one untimed run (code objects, descriptors), then `windows` timed windows of `runs` network.run(time) calls (`host-runs` on
the host path: either way a window lasts about a second), each call followed by reset_state_variables(), each window closed by a
device synchronise; prints one JSON line with the median and the
spread (min, max) of the windows' timesteps/s.  A device row fails where there is no GPU; nothing falls back.  The kernel shape is
the fused one (draw + update in one workgroup, csrc/snn_srm0.hip); under `rocprofv3 --kernel-trace --stats -- python
tools/bench_srm0.py --no-host` k_srm0 and k_rmax show once per timestep."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def graph(rule: bool, seed=0):
    from bindsnet_amd.learning import Rmax
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, SRM0Nodes
    from bindsnet_amd.network.topology import Connection
    rng = np.random.default_rng(seed)
    net = Network()
    X, Y = Input(n=784, traces=True, traces_additive=True), SRM0Nodes(n=100, traces=True)
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    w = torch.from_numpy((rng.random((784, 100), dtype=np.float32) * np.float32(0.05)).astype(np.float32))
    kw = dict(update_rule=Rmax, nu=1e-4, wmin=0.0, wmax=0.1) if rule else {}
    net.add_connection(Connection(X, Y, w=w, **kw), "X", "Y")
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=300, help="network.run() calls per timed window on the device (about a second)")
    ap.add_argument("--host-runs", type=int, default=16, help="the same on the host path")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    rows = [("rmax", True, 1), ("plain", False, 1), ("plain", False, 16)]
    for dev in ["cuda:0"] + ([] if a.no_host else ["cpu"]):
        for label, rule, B in rows:
            torch.manual_seed(0)
            net = graph(rule).to(dev)
            x = torch.from_numpy((np.random.default_rng(1).random((a.time, B, 784)) < 0.05).astype(np.uint8)).to(dev)
            kw = {"reward": 1.0} if rule else {}
            sync = torch.cuda.synchronize if dev != "cpu" else (lambda: None)
            net.run({"X": x}, time=a.time, **kw)
            net.reset_state_variables()
            sync()
            runs = a.host_runs if dev == "cpu" else a.runs
            rates, secs = [], []
            for _ in range(a.windows):
                t0 = time.perf_counter()
                for _ in range(runs):
                    net.run({"X": x}, time=a.time, **kw)
                    net.reset_state_variables()
                sync()
                secs.append(time.perf_counter() - t0)
                rates.append(runs * a.time / secs[-1])
            print(json.dumps({"graph": "Input 784 -> Connection -> SRM0Nodes 100", "row": label, "device": dev, "plan": net.last_plan, "B": B,
                              "T": a.time, "windows": a.windows, "runs_per_window": runs, "window_s": round(statistics.median(secs), 3), "kernel_shape": "fused draw + update",
                              "timesteps_per_s_median": round(statistics.median(rates), 1), "timesteps_per_s_min": round(min(rates), 1),
                              "timesteps_per_s_max": round(max(rates), 1)}), flush=True)


if __name__ == "__main__":
    main()
