#!/usr/bin/env python3
"""What the state monitors cost on the MI355X: timesteps/s of

    Input 784 -> Weight + PostPre -> DiehlAndCookNodes 400, B = 32, T = 250, synchronous runs

with four sets of monitors on the target layer:

    sv        s + v                                   (none of the state-monitor code runs)
    x         s + v + x                               (one snn_record_segments launch per timestep, one segment)
    xtr       s + v + x + theta + refrac_count        (the same launch, three segments)
    activity  the same, the connection built with traces=True and its `activity` monitored
              (propagation into the activity buffer, one k_feed_activity launch, four segments)

    python tools/bench_state_monitors.py [--time 250] [--windows 5] [--runs 10] [--rows sv x xtr activity] [--label TEXT]

The process-wide switch holds every row on the generic plan (the `sv` graph alone would match a one-launch plan), so the rows differ
in the monitors only.  Per row: one untimed run, then `windows` timings of `runs` network.run(time) calls on 10 %-dense Bernoulli
input, each followed by reset_state_variables(), end to end with the device synchronised; weights and adaptive thresholds go back
to their initial values before every window.  Prints one JSON line per row with every window, the median and the min-max spread,
then the ratios of the other medians over `sv`'s.  `--rows sv` runs on a commit from before the state monitors as well: run it on
two commits in one session, alternating, to compare them."""
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

S, N, B = 784, 400, 32
ROWS = {"sv": ("s", "v"), "x": ("s", "v", "x"), "xtr": ("s", "v", "x", "theta", "refrac_count"),
        "activity": ("s", "v", "x", "theta", "refrac_count")}


def build(row, T):
    from bindsnet_amd.learning.MCC_learning import PostPre
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.monitors import Monitor
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input
    from bindsnet_amd.network.topology import MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Weight
    torch.manual_seed(0)
    net = Network(dt=1.0, learning=True)
    X = Input(n=S, traces=True)
    Y = DiehlAndCookNodes(n=N, traces=True, theta_plus=0.05, tc_theta_decay=1e7)
    w = torch.from_numpy(np.float32(0.02) + np.random.default_rng(4).random((S, N), dtype=np.float32) * np.float32(0.28))
    feat = Weight("weight", w, range=[0.0, 1.0], norm=78.4, nu=[1e-4, 1e-2], reduction=torch.sum, learning_rule=PostPre)
    kw = dict(traces=True) if row == "activity" else {}
    conn = MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat], **kw)
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(conn, "X", "Y")
    net.add_monitor(Monitor(Y, list(ROWS[row]), time=T), "Y")
    if row == "activity":
        net.add_monitor(Monitor(conn, ["activity"], time=T), "activity")
    return net.to("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rows", nargs="+", default=list(ROWS), choices=list(ROWS))
    ap.add_argument("--label", default="", help="copied into every JSON line (which commit the rows belong to)")
    a = ap.parse_args()
    from bindsnet_amd import _lib
    _lib.lib().snn_set_plan_mode(1)                    # the generic plan for the `sv` row as well
    x = torch.from_numpy((np.random.default_rng(2).random((a.time, B, S)) < 0.1).astype(np.uint8)).to("cuda:0")
    medians = {}
    for row in a.rows:
        net = build(row, a.time)
        feat = net.connections[("X", "Y")].pipeline[0]
        w0 = feat.value.detach().clone()
        torch.manual_seed(3)
        net.run({"X": x}, time=a.time)
        net.reset_state_variables()
        torch.cuda.synchronize()
        rates = []
        for _ in range(a.windows):
            feat.value.data.copy_(w0)
            net.layers["Y"].theta.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.runs):
                net.run({"X": x}, time=a.time)
                net.reset_state_variables()
            torch.cuda.synchronize()
            rates.append(a.runs * a.time / (time.perf_counter() - t0))
        medians[row] = statistics.median(rates)
        print(json.dumps({"label": a.label, "row": row, "monitors": list(ROWS[row]) + (["activity"] if row == "activity" else []),
                          "plan": net.last_plan, "S": S, "N": N, "B": B, "T": a.time, "runs_per_window": a.runs,
                          "timesteps_per_s": [round(r, 1) for r in rates], "median": round(medians[row], 1),
                          "min": round(min(rates), 1), "max": round(max(rates), 1)}), flush=True)
    if "sv" in medians and len(medians) > 1:
        print(json.dumps({"label": a.label, **{f"{m}_over_sv": round(v / medians["sv"], 4) for m, v in medians.items() if m != "sv"}}),
              flush=True)


if __name__ == "__main__":
    main()
