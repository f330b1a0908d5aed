#!/usr/bin/env python3
"""Timesteps/s of the examples/mnist/MCC_reservoir.py graph -- Input 784 -> LIFNodes 500 (per-neuron thresholds) -> itself, both
connections MulticompartmentConnection [Probability, Weight], B = 1, T = 250 -- on the MI355X (generic plan) and on the host path of
the same machine.

    python tools/bench_mcc_reservoir.py [--time 250] [--runs 3] [--host-runs 1]

Per timestep the graph draws 784*500 + 500*500 = 642 000 consecutive mt19937 outputs (about 1 029 twists of the 624-word state)
from the host generator's stream: a serial chain on either side.  One untimed run, then `runs` network.run(time) calls on
Bernoulli input, each followed by reset_state_variables(), timed end to end with the device synchronised; prints one JSON line
per side.  Both sides start from the same seed, so the device line also says whether its raster equals the host's."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def reservoir(n_in=784, n=500, seed=0):
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Probability, Weight
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    net = Network(dt=1.0)
    X = Input(n=n_in, traces=True)
    Y = LIFNodes(n=n, thresh=torch.from_numpy((-52.0 + rng.standard_normal(n)).astype(np.float32)), traces=True)
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    for (a, b), name in (((X, Y), "input"), ((Y, Y), "recc")):       # MCC_reservoir.py:93-117: p uniform, w the sign of randint(-1, 2)
        p = torch.rand(a.n, b.n)
        w = torch.sign(torch.randint(-1, 2, (a.n, b.n))).float()
        net.add_connection(MulticompartmentConnection(a, b, device="cpu", pipeline=[Probability(name + "_prob_feature", p),
                                                                                    Weight(name + "_weight_feature", w)]),
                           "X" if a is X else "Y", "Y")
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--density", type=float, default=0.1)
    a = ap.parse_args()
    from bindsnet_amd.network.monitors import Monitor
    x = torch.from_numpy((np.random.default_rng(1).random((a.time, 1, 784)) < a.density).astype(np.uint8))
    first = {}
    for side, runs in (("host", a.host_runs), ("device", a.runs)):
        dev = "cuda:0" if side == "device" else "cpu"
        net = reservoir()
        mon = Monitor(net.layers["Y"], ["s"], time=a.time)
        net.add_monitor(mon, "Y")
        net.to(dev)
        xd = x.to(dev)
        torch.manual_seed(7)
        net.run({"X": xd.clone()}, time=a.time)              # untimed; both sides from the same generator state
        first[side] = mon.get("s").cpu().numpy().copy()
        net.reset_state_variables()
        if side == "device":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(runs):
            net.run({"X": xd.clone()}, time=a.time)
            net.reset_state_variables()
        if side == "device":
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        line = {"graph": "MCC_reservoir.py shape (784 -> 500 + 500 -> 500, [Probability, Weight], per-neuron thresholds)", "side": side,
                "plan": net.last_plan, "B": 1, "T": a.time, "runs": runs, "timesteps_per_s": round(runs * a.time / dt, 1),
                "ms_per_timestep": round(1e3 * dt / (runs * a.time), 4), "spikes_first_run": int(first[side].sum()),
                "draws_per_timestep": 784 * 500 + 500 * 500, "host_threads": torch.get_num_threads()}
        if side == "device":
            line["raster_equals_host"] = bool(np.array_equal(first["host"], first["device"]))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
