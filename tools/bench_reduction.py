#!/usr/bin/env python3
"""Timesteps/s of two learning graphs on the MI355X, generic plan, under the batch reductions torch.sum, torch.mean and torch.amax
(include/snnhip.h f15):

    mcc     Input 784 -> Weight + PostPre     -> DiehlAndCookNodes 400, B = 32
    dense   Input 784 -> Connection + PostPre -> LIFNodes 400,          B = 16

    python tools/bench_reduction.py [--time 250] [--windows 5] [--runs 10] [--graphs mcc dense] [--reductions sum mean amax]

The sum graphs would match a one-launch plan; the process-wide switch is set to the generic plan, so that all rows time the same
launches around the rule (sum: k_plasticity, mean / amax: k_plasticity_red with the accumulator exchanged -- one division per element
and step more, or a compare in an add's place).

Per graph and reduction: one untimed run, then `windows` timings of `runs` network.run(time) calls on 10 %-dense Bernoulli input, each
followed by reset_state_variables(), end to end with the device synchronised; weights and adaptive thresholds go back to their
initial values before every window, so that the windows time the same activity.  Prints one JSON line each with every window, the
median and the min-max spread, and per graph the ratios of the other medians over sum's.  The sum rows run the kernels they ran before
these reductions existed: run `--reductions sum` on two commits in one session, alternating, to compare them."""
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

GRAPHS = {"mcc": dict(B=32), "dense": dict(B=16)}
REDUCTIONS = {"sum": torch.sum, "mean": torch.mean, "amax": torch.amax, "amin": torch.amin}
S, N = 784, 400


def build(graph, reduction):
    from bindsnet_amd.learning import PostPre
    from bindsnet_amd.learning.MCC_learning import PostPre as MCCPostPre
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input, LIFNodes
    from bindsnet_amd.network.topology import Connection, MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Weight
    torch.manual_seed(0)
    net = Network(dt=1.0, learning=True)
    X = Input(n=S, traces=True)
    w = torch.from_numpy(np.float32(0.02) + np.random.default_rng(4).random((S, N), dtype=np.float32) * np.float32(0.28))
    if graph == "mcc":
        Y = DiehlAndCookNodes(n=N, traces=True, theta_plus=0.05, tc_theta_decay=1e7)
        feat = Weight("weight", w, range=[0.0, 1.0], norm=78.4, nu=[1e-4, 1e-2], reduction=REDUCTIONS[reduction], learning_rule=MCCPostPre)
        conn = MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat])
    else:
        Y = LIFNodes(n=N, traces=True)
        conn = Connection(X, Y, w=w, wmin=0.0, wmax=1.0, norm=78.4, nu=[1e-4, 1e-2], reduction=REDUCTIONS[reduction], update_rule=PostPre)
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(conn, "X", "Y")
    return net.to("cuda:0")


def weights(net):
    conn = net.connections[("X", "Y")]
    return conn.pipeline[0].value if hasattr(conn, "pipeline") else conn.w


def restore(net, w0):
    weights(net).data.copy_(w0)
    theta = getattr(net.layers["Y"], "theta", None)
    if theta is not None:
        theta.zero_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--graphs", nargs="+", default=list(GRAPHS), choices=list(GRAPHS))
    ap.add_argument("--reductions", nargs="+", default=["sum", "mean", "amax"], choices=list(REDUCTIONS))
    ap.add_argument("--label", default="", help="copied into every JSON line (which commit the rows belong to)")
    a = ap.parse_args()
    from bindsnet_amd import _lib
    _lib.lib().snn_set_plan_mode(1)                    # the generic plan for the sum rows as well
    for graph in a.graphs:
        B = GRAPHS[graph]["B"]
        x = torch.from_numpy((np.random.default_rng(2).random((a.time, B, S)) < 0.1).astype(np.uint8)).to("cuda:0")
        medians = {}
        for reduction in a.reductions:
            net = build(graph, reduction)
            w0 = weights(net).detach().clone()
            torch.manual_seed(3)
            net.run({"X": x}, time=a.time)
            net.reset_state_variables()
            torch.cuda.synchronize()
            rates = []
            for _ in range(a.windows):
                restore(net, w0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.runs):
                    net.run({"X": x}, time=a.time)
                    net.reset_state_variables()
                torch.cuda.synchronize()
                rates.append(a.runs * a.time / (time.perf_counter() - t0))
            medians[reduction] = statistics.median(rates)
            print(json.dumps({"label": a.label, "graph": graph, "reduction": reduction, "plan": net.last_plan, "S": S, "N": N, "B": B,
                              "T": a.time, "runs_per_window": a.runs, "timesteps_per_s": [round(r, 1) for r in rates],
                              "median": round(medians[reduction], 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}), flush=True)
        if "sum" in medians and len(medians) > 1:
            print(json.dumps({"label": a.label, "graph": graph,
                              **{f"{m}_over_sum": round(v / medians["sum"], 4) for m, v in medians.items() if m != "sum"}}), flush=True)


if __name__ == "__main__":
    main()
