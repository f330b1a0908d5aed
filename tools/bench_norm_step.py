#!/usr/bin/env python3
"""Timesteps/s of Input 784 -> Weight + PostPre (norm 78.4) -> DiehlAndCookNodes 400, B = 32, on the MI355X, generic plan, under the
two normalisation frequencies of a Weight (include/snnhip.h f16):

    sample          norm_frequency="sample": one normalisation at the end of run()
    step_fused      norm_frequency="time step" through snn_prop_cascade_norm_f32: propagation and normalisation in one launch
    step_two_calls  norm_frequency="time step" through snn_prop_cascade_f32 + snn_normalize: three launches

    python tools/bench_norm_step.py [--time 250] [--windows 5] [--runs 10] [--rows sample step_fused step_two_calls]

The sample graph would match a one-launch plan; the process-wide switch is set to the generic plan, so that all rows time the same
launches around the normalisation.  Per row: one untimed run, then `windows` timings of `runs` network.run(time) calls on 10 %-dense
Bernoulli input, each followed by reset_state_variables(), end to end with the device synchronised; weights and adaptive thresholds
go back to their initial values before every window.  Prints one JSON line per row with every window, the median, the min-max
spread and the output layer's spike count of one run.  The two step rows compute the same bits, so their ratio is the cost of the
launches; the sample row learns OTHER weights (its spike count differs), so its ratio to a step row is not the cost of the feature.
The sample row runs the kernels it ran before this mode existed: run `--rows sample` on two commits in one session, alternating, to
compare them."""
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
ROWS = {"sample": ("sample", None), "step_fused": ("time step", 2), "step_two_calls": ("time step", 1)}


def build(row):
    from bindsnet_amd.learning.MCC_learning import PostPre
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input
    from bindsnet_amd.network.topology import MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Weight
    frequency, form = ROWS[row]
    torch.manual_seed(0)
    net = Network(dt=1.0, learning=True)
    X = Input(n=S, traces=True)
    Y = DiehlAndCookNodes(n=N, traces=True, theta_plus=0.05, tc_theta_decay=1e7)
    w = torch.from_numpy(np.float32(0.02) + np.random.default_rng(4).random((S, N), dtype=np.float32) * np.float32(0.28))
    kw = {} if frequency == "sample" else {"norm_frequency": frequency}        # (a commit without the mode takes the sample row)
    feat = Weight("weight", w, range=[0.0, 1.0], norm=78.4, nu=[1e-4, 1e-2], reduction=torch.sum, learning_rule=PostPre, **kw)
    conn = MulticompartmentConnection(X, Y, device="cpu", pipeline=[feat])
    if form is not None:
        conn._NORM_STEP_FORM = form
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(conn, "X", "Y")
    return net.to("cuda:0")


def restore(net, w0):
    net.connections[("X", "Y")].pipeline[0].value.data.copy_(w0)
    net.layers["Y"].theta.zero_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rows", nargs="+", default=list(ROWS), choices=list(ROWS))
    ap.add_argument("--label", default="", help="copied into every JSON line (which commit the rows belong to)")
    a = ap.parse_args()
    from bindsnet_amd import _lib
    from bindsnet_amd.network.monitors import Monitor
    _lib.lib().snn_set_plan_mode(1)                    # the generic plan for the sample row as well
    x = torch.from_numpy((np.random.default_rng(2).random((a.time, B, S)) < 0.1).astype(np.uint8)).to("cuda:0")
    medians = {}
    for row in a.rows:
        net = build(row)
        w0 = net.connections[("X", "Y")].pipeline[0].value.detach().clone()
        mon = Monitor(net.layers["Y"], ["s"], time=a.time)
        net.add_monitor(mon, "Y_s")
        torch.manual_seed(3)
        net.run({"X": x}, time=a.time)
        spikes = int(mon.get("s").sum())
        del net.monitors["Y_s"]
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
        medians[row] = statistics.median(rates)
        print(json.dumps({"label": a.label, "row": row, "plan": net.last_plan, "S": S, "N": N, "B": B, "T": a.time,
                          "runs_per_window": a.runs, "spikes_first_run": spikes, "timesteps_per_s": [round(r, 1) for r in rates],
                          "median": round(medians[row], 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}), flush=True)
    if "step_fused" in medians and "step_two_calls" in medians:
        print(json.dumps({"label": a.label, "fused_over_two_calls": round(medians["step_fused"] / medians["step_two_calls"], 4)}), flush=True)


if __name__ == "__main__":
    main()
