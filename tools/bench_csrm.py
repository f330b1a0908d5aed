#!/usr/bin/env python3
"""Per-step time of a CSRM graph on the MI355X: Input -> Connection (PostPre nu 1e-2) -> CSRMNodes, T = 250, at

    100 -> 100   (the graph of the reference's test/network/test_learning.py)      B = 1 and 32
    784 -> 400                                                                     B = 1 and 32

and, for scale, the same graphs with an LIFNodes target on the same tree (whatever plan the library picks for them).

    python tools/bench_csrm.py [--time 250] [--windows 5] [--runs 40]

Per row: one untimed run (code objects, descriptors), then `windows` timed windows of `runs` network.run(time) calls, each call
followed by reset_state_variables(), each window closed by a device synchronise; prints one JSON line with the plan, the median
microseconds per timestep and the spread (min, max) over the windows.  Fails where there is no GPU; nothing falls back.  The input
density is 10 %, so a window of 20 slots holds about 2 * n_src spikes: by the shapes the windowed propagation gathers about 20
times the rows a plain connection's does (an expectation, not something this tool measures)."""
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


def graph(n_src: int, n: int, B: int, csrm: bool, seed=0):
    from bindsnet_amd.learning import PostPre
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import CSRMNodes, Input, LIFNodes
    from bindsnet_amd.network.topology import Connection
    rng = np.random.default_rng(seed)
    net = Network(batch_size=B)
    X = Input(n=n_src, traces=True)
    Y = CSRMNodes(n=n, traces=True) if csrm else LIFNodes(n=n, traces=True)
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    w = torch.from_numpy((rng.random((n_src, n)) * 30.0 / n_src).astype(np.float32))
    net.add_connection(Connection(X, Y, w=w, update_rule=PostPre, nu=1e-2, wmin=0.0, wmax=1.0), "X", "Y")
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=40, help="network.run() calls per timed window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_csrm.py needs an MI355X")
    dev = "cuda:0"
    for n_src, n in ((100, 100), (784, 400)):
        for B in (1, 32):
            for csrm in (True, False):
                net = graph(n_src, n, B, csrm).to(dev)
                rng = np.random.default_rng(1)
                x = torch.from_numpy((rng.random((a.time, B, n_src)) < 0.1).astype(np.uint8)).to(dev)

                def once():
                    net.run({"X": x}, time=a.time)
                    net.reset_state_variables()

                once()
                torch.cuda.synchronize()
                us = []
                for _ in range(a.windows):
                    t0 = time.perf_counter()
                    for _ in range(a.runs):
                        once()
                    torch.cuda.synchronize()
                    us.append((time.perf_counter() - t0) * 1e6 / (a.runs * a.time))
                print(json.dumps({"graph": f"{n_src}->{n}", "target": "CSRMNodes" if csrm else "LIFNodes", "B": B, "plan": net.last_plan,
                                  "us_per_step_median": round(statistics.median(us), 3), "us_per_step_min": round(min(us), 3),
                                  "us_per_step_max": round(max(us), 3)}), flush=True)


if __name__ == "__main__":
    main()
