#!/usr/bin/env python3
"""Timesteps/s of two graphs on the MI355X, generic plan, each with all-scalar node parameters and with every supported parameter
given as a tensor with one value per neuron (include/snnhip.h f10); traces are additive, so that trace_scale is among them:

    lif   Input 784 -> MulticompartmentConnection + Weight -> LIFNodes 1600, B = 16  (thresh, tc_decay, tc_trace, trace_scale)
    dc    Input 784 -> MulticompartmentConnection + Weight -> DiehlAndCookNodes 400, B = 32
                                                  (thresh, tc_decay, tc_trace, trace_scale, theta_plus, tc_theta_decay)

    python tools/bench_hetero.py [--time 250] [--repeats 5] [--runs 10] [--graphs lif dc] [--modes scalar uniform tensor]

Modes: `scalar`; `uniform`, every parameter a tensor filled with the scalar row's value -- the same network, spike for spike, so
uniform over scalar is the cost of the per-neuron kernel instances alone; `tensor`, values spread around the scalar row's, which
also changes the activity.  The weights are the same in every mode.

The scalar graphs would match a fused plan; the per-run plan request is left alone and the process-wide switch is set to the
generic plan, so that both rows time the same launches.  Per graph and mode: one untimed run, then `repeats` timings of `runs`
network.run(time) calls on 10 %-dense Bernoulli input, each followed by reset_state_variables(), end to end with the device
synchronised; the adaptive thresholds `theta`, which reset_state_variables() leaves alone, go back to zero before every repeat, so that
the repeats time the same activity; prints one JSON line each with every repeat, the median and the min-max spread, and for each
graph the ratios of the uniform and tensor medians over the scalar one."""
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

GRAPHS = {"lif": dict(n=1600, B=16), "dc": dict(n=400, B=32)}


def build(graph, mode):
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input, LIFNodes
    from bindsnet_amd.network.topology import MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Weight
    n = GRAPHS[graph]["n"]
    rng = np.random.default_rng(1)

    def par(lo, hi):
        """One value per neuron, or -- scalar mode -- the middle of the range."""
        spread = (lo + (hi - lo) * rng.random(n, dtype=np.float32)).astype(np.float32)     # (drawn in every mode)
        mid = 0.5 * (lo + hi)
        return {"scalar": mid, "uniform": torch.full((n,), mid), "tensor": torch.from_numpy(spread)}[mode]

    torch.manual_seed(0)
    net = Network(dt=1.0, learning=True)
    X = Input(n=784, traces=True)
    kw = dict(n=n, traces=True, traces_additive=True, thresh=par(-56.0, -48.0), tc_decay=par(60.0, 140.0), tc_trace=par(10.0, 30.0),
              trace_scale=par(0.5, 1.5))
    Y = LIFNodes(**kw) if graph == "lif" else DiehlAndCookNodes(theta_plus=par(0.02, 0.08), tc_theta_decay=par(1e3, 1e4), **kw)
    w = torch.from_numpy(np.random.default_rng(4).random((784, n), dtype=np.float32) * np.float32(0.3))
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(MulticompartmentConnection(X, Y, device="cpu", pipeline=[Weight("weight", w)]), "X", "Y")
    return net.to("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--graphs", nargs="+", default=["lif", "dc"], choices=sorted(GRAPHS))
    ap.add_argument("--modes", nargs="+", default=["scalar", "uniform", "tensor"], choices=["scalar", "uniform", "tensor"])
    a = ap.parse_args()
    from bindsnet_amd import _lib
    _lib.lib().snn_set_plan_mode(1)                    # the generic plan for the scalar rows as well
    for graph in a.graphs:
        B = GRAPHS[graph]["B"]
        x = torch.from_numpy((np.random.default_rng(2).random((a.time, B, 784)) < 0.1).astype(np.uint8)).to("cuda:0")
        medians = {}
        for mode in a.modes:
            net = build(graph, mode)
            theta = getattr(net.layers["Y"], "theta", None)
            torch.manual_seed(3)
            net.run({"X": x}, time=a.time)
            net.reset_state_variables()
            torch.cuda.synchronize()
            rates = []
            for _ in range(a.repeats):
                if theta is not None:
                    theta.zero_()
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.runs):
                    net.run({"X": x}, time=a.time)
                    net.reset_state_variables()
                torch.cuda.synchronize()
                rates.append(a.runs * a.time / (time.perf_counter() - t0))
            medians[mode] = statistics.median(rates)
            print(json.dumps({"graph": graph, "mode": mode, "plan": net.last_plan, "n": GRAPHS[graph]["n"], "B": B, "T": a.time,
                              "runs_per_repeat": a.runs, "timesteps_per_s": [round(r, 1) for r in rates],
                              "median": round(medians[mode], 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}), flush=True)
        if "scalar" in medians and len(medians) > 1:
            print(json.dumps({"graph": graph, **{f"{m}_over_scalar": round(v / medians["scalar"], 4) for m, v in medians.items() if m != "scalar"}}),
                  flush=True)


if __name__ == "__main__":
    main()
