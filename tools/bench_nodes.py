#!/usr/bin/env python3
"""Timesteps/s of the breakout.py graph shape (tests/node_cases.py breakout_graph: Input 6400 -> Connection (MSTDP) -> 100 hidden
-> Connection (MSTDP) -> 4 output neurons, reward 1.0) on the MI355X, generic plan, learning on: once with IzhikevichNodes in
both layers, as the example has them, and once with LIFNodes -- the same graph from layers every version of the package has.

    python tools/bench_nodes.py [--time 250] [--batch 1 16] [--runs 5]

Per layer kind and batch size: one untimed run, then `runs` network.run(time) calls on 2 %-dense Bernoulli input, each followed
by reset_state_variables(), timed end to end with the device synchronised; prints one JSON line each.  Under
`rocprofv3 --kernel-trace --stats -- python tools/bench_nodes.py` the Izhikevich rows show k_izh launched once per layer and
timestep."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--hidden", nargs="+", default=["izh", "lif"], choices=["izh", "lif"])
    a = ap.parse_args()
    import node_cases as NC
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network, nodes, topology
    for hidden in a.hidden:
        for B in a.batch:
            net = NC.breakout_graph(nodes, topology, learning, Network, hidden).to("cuda:0")
            x = torch.from_numpy(NC.breakout_input(a.time, B)).to("cuda:0")
            net.run({"X": x}, time=a.time, reward=1.0)
            net.reset_state_variables()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.runs):
                net.run({"X": x}, time=a.time, reward=1.0)
                net.reset_state_variables()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"graph": "breakout shape (6400 -> 100 -> 4, dense Connection + MSTDP)", "hidden": hidden, "plan": net.last_plan,
                              "B": B, "T": a.time, "runs": a.runs, "timesteps_per_s": round(a.runs * a.time / dt, 1),
                              "sample_timesteps_per_s": round(a.runs * a.time * B / dt, 1), "ms_per_run": round(1e3 * dt / a.runs, 3)}))


if __name__ == "__main__":
    main()
