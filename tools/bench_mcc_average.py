#!/usr/bin/env python3
"""Timesteps/s of two MulticompartmentConnection learning graphs on the MI355X, generic plan, each with the plain rule and with
time-averaged updates (average_update = 10; include/snnhip.h f14) in both modes:

    postpre  Input 784 -> Weight + PostPre -> DiehlAndCookNodes 400, B = 32
    mstdp    Input 784 -> Weight + MSTDP   -> LIFNodes 400, B = 16 (reward 1.0)

    python tools/bench_mcc_average.py [--time 250] [--windows 5] [--runs 10] [--graphs postpre mstdp] [--modes plain windowed continuous]

Modes: `plain` (average_update = 0: snn_stdp_postpre / snn_mstdp_step), `windowed` (K = 10, continues_update=False: the ring's mean is
read every tenth step) and `continuous` (K = 10, continues_update=True: every step reads the K slots).  The plain graphs would match a
fused plan; the process-wide switch is set to the generic plan, so that all rows time the same launches around the rule.

Per graph and mode: one untimed run, then `windows` timings of `runs` network.run(time) calls on 10 %-dense Bernoulli input, each
followed by reset_state_variables(), end to end with the device synchronised; weights, adaptive thresholds, rings and ring indices
go back to their initial values before every window, so that the windows time the same activity.  Prints one JSON line each with
every window, the median and the min-max spread, and per graph the ratios of the averaged medians over the plain one.  The plain
rows share no kernel with the averaged ones: run `--modes plain` on two commits in one session to compare them."""
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

GRAPHS = {"postpre": dict(B=32), "mstdp": dict(B=16)}
MODES = {"plain": {}, "windowed": dict(average_update=10, continues_update=False), "continuous": dict(average_update=10, continues_update=True)}
S, N = 784, 400


def build(graph, mode):
    from bindsnet_amd.learning.MCC_learning import MSTDP, PostPre
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input, LIFNodes
    from bindsnet_amd.network.topology import MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Weight
    torch.manual_seed(0)
    net = Network(dt=1.0, learning=True)
    X = Input(n=S, traces=True)
    w = torch.from_numpy(np.float32(0.02) + np.random.default_rng(4).random((S, N), dtype=np.float32) * np.float32(0.28))
    if graph == "postpre":
        Y = DiehlAndCookNodes(n=N, traces=True, theta_plus=0.05, tc_theta_decay=1e7)
        feat = Weight("weight", w, range=[0.0, 1.0], norm=78.4, nu=[1e-4, 1e-2], reduction=torch.sum, learning_rule=PostPre)
    else:
        Y = LIFNodes(n=N, traces=True)
        feat = Weight("weight", w, range=[0.0, 1.0], norm=78.4, nu=[1e-4, 0.0], reduction=torch.sum, learning_rule=MSTDP)
    conn = MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat], **MODES[mode])
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(conn, "X", "Y")
    return net.to("cuda:0")


def restore(net, w0):
    """Weights, thresholds, rings and indices as they were before the first run."""
    feat = net.connections[("X", "Y")].pipeline[0]
    feat.value.data.copy_(w0)
    theta = getattr(net.layers["Y"], "theta", None)
    if theta is not None:
        theta.zero_()
    rule = feat.learning_rule
    for name in ("average_buffer", "average_buffer_pre", "average_buffer_post"):
        if hasattr(rule, name):
            getattr(rule, name).zero_()
    for name in ("average_buffer_index", "average_buffer_index_pre", "average_buffer_index_post"):
        if hasattr(rule, name):
            setattr(rule, name, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--graphs", nargs="+", default=sorted(GRAPHS), choices=sorted(GRAPHS))
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    ap.add_argument("--label", default="", help="copied into every JSON line (which commit the rows belong to)")
    a = ap.parse_args()
    from bindsnet_amd import _lib
    _lib.lib().snn_set_plan_mode(1)                    # the generic plan for the plain rows as well
    for graph in a.graphs:
        B = GRAPHS[graph]["B"]
        x = torch.from_numpy((np.random.default_rng(2).random((a.time, B, S)) < 0.1).astype(np.uint8)).to("cuda:0")
        kw = {"reward": 1.0} if graph == "mstdp" else {}
        medians = {}
        for mode in a.modes:
            net = build(graph, mode)
            w0 = net.connections[("X", "Y")].pipeline[0].value.detach().clone()
            torch.manual_seed(3)
            net.run({"X": x}, time=a.time, **kw)
            net.reset_state_variables()
            torch.cuda.synchronize()
            rates = []
            for _ in range(a.windows):
                restore(net, w0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.runs):
                    net.run({"X": x}, time=a.time, **kw)
                    net.reset_state_variables()
                torch.cuda.synchronize()
                rates.append(a.runs * a.time / (time.perf_counter() - t0))
            medians[mode] = statistics.median(rates)
            print(json.dumps({"label": a.label, "graph": graph, "mode": mode, "plan": net.last_plan, "S": S, "N": N, "B": B, "T": a.time,
                              "runs_per_window": a.runs, "timesteps_per_s": [round(r, 1) for r in rates],
                              "median": round(medians[mode], 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}), flush=True)
        if "plain" in medians and len(medians) > 1:
            print(json.dumps({"label": a.label, "graph": graph,
                              **{f"{m}_over_plain": round(v / medians["plain"], 4) for m, v in medians.items() if m != "plain"}}), flush=True)


if __name__ == "__main__":
    main()
