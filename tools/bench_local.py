#!/usr/bin/env python3
"""Timesteps/s of the loc2d_mnist.py graph (tests/local_cases.py case (a): Input [1, 20, 20] -> LocalConnection2D k 12 s 4,
50 filters, PostPre -> AdaptiveLIFNodes [50, 3, 3] with the recurrent inhibition) on the MI355X, generic plan, learning on.

    python tools/bench_local.py [--time 250] [--batch 1 32] [--runs 5]

Per batch size: one untimed run, then `runs` network.run(time) calls on 5 %-dense random input, each followed by
reset_state_variables(), timed end to end with the device synchronised; prints one JSON line per batch size."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import local_cases as LC
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network, nodes, topology
    ns = LC.ns_from(nodes, topology, learning, Network)
    for B in a.batch:
        net = LC.build(ns, "a").to("cuda:0")
        rng = np.random.default_rng(B)
        x = torch.from_numpy((rng.random((a.time, B, 1, 20, 20)) < 0.05).astype(np.uint8)).to("cuda:0")
        net.run({"X": x}, time=a.time)
        net.reset_state_variables()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.runs):
            net.run({"X": x}, time=a.time)
            net.reset_state_variables()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"graph": "loc2d (LocalConnection2D PostPre + AdaptiveLIF + recurrent inhibition)", "plan": net.last_plan,
                          "B": B, "T": a.time, "runs": a.runs, "timesteps_per_s": round(a.runs * a.time / dt, 1),
                          "sample_timesteps_per_s": round(a.runs * a.time * B / dt, 1), "ms_per_run": round(1e3 * dt / a.runs, 3)}))


if __name__ == "__main__":
    main()
