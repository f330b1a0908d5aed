#!/usr/bin/env python3
"""Timesteps/s of two learning graphs on the MI355X, generic plan, each with scalar learning rates, weight bounds and norm and with
those constants given as tensors (include/snnhip.h f13):

    dense  Input 784 -> Connection + PostPre -> LIFNodes 400, B = 16              (nu [N] pair, wmin / wmax [S, N], norm [N])
    mcc    Input 784 -> MulticompartmentConnection + Weight + PostPre -> DiehlAndCookNodes 400, B = 32
                                                                                  (range [S, N] pair, norm [N]; MCC rates stay scalar)

    python tools/bench_synparams.py [--time 250] [--repeats 5] [--runs 10] [--graphs dense mcc] [--modes scalar uniform tensor]

Modes: `scalar`; `uniform`, every constant a tensor filled with the scalar row's value -- the same network spike for spike apart from
the rounding of the norm (a tensor norm divides, a float multiplies by the reciprocal), so uniform over scalar is the cost of the
per-synapse kernel instances alone; `tensor`, values spread around the scalar row's.

The scalar graphs would match a fused plan; the process-wide switch is set to the generic plan, so that all rows time the same
launches.  Per graph and mode: one untimed run, then `repeats` timings of `runs` network.run(time) calls on 10 %-dense Bernoulli
input, each followed by reset_state_variables(), end to end with the device synchronised; weights (and the adaptive thresholds)
go back to their initial values before every repeat, so that the repeats time the same activity.  Prints one JSON line each with
every repeat, the median and the min-max spread, and for each graph the ratios of the uniform and tensor medians over the scalar one.

`build()` is also imported by tests/test_gpu_synparams.py, which runs the dense graph WITHOUT the plan switch to see that its scalar
form keeps the one-launch plan and its tensor forms take the generic one: keep its signature and the dense graph's shape."""
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

GRAPHS = {"dense": dict(B=16), "mcc": dict(B=32)}
S, N = 784, 400


def build(graph, mode):
    from bindsnet_amd.learning import PostPre
    from bindsnet_amd.learning.MCC_learning import PostPre as MccPostPre
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import DiehlAndCookNodes, Input, LIFNodes
    from bindsnet_amd.network.topology import Connection, MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Weight
    rng = np.random.default_rng(1)

    def par(shape, lo, hi):
        """A constant of `shape`, or -- scalar mode -- the middle of the range."""
        spread = (lo + (hi - lo) * rng.random(shape, dtype=np.float32)).astype(np.float32)     # (drawn in every mode)
        mid = 0.5 * (lo + hi)
        return {"scalar": mid, "uniform": torch.full(shape, mid), "tensor": torch.from_numpy(spread)}[mode]

    torch.manual_seed(0)
    net = Network(dt=1.0, learning=True)
    X = Input(n=S, traces=True)
    w = torch.from_numpy(np.float32(0.02) + np.random.default_rng(4).random((S, N), dtype=np.float32) * np.float32(0.28))   # (inside every range below)
    lo, hi, norm = par((S, N), 0.0, 0.02), par((S, N), 0.8, 1.2), par((N,), 60.0, 96.0)
    if graph == "dense":
        Y = LIFNodes(n=N, traces=True)
        nu0, nu1 = par((N,), 5e-5, 1.5e-4), par((N,), 5e-3, 1.5e-2)
        nu = (nu0, nu1) if mode == "scalar" else [nu0, nu1]
        conn = Connection(X, Y, w=w, wmin=lo, wmax=hi, norm=norm, update_rule=PostPre, nu=nu, reduction=torch.sum)
    else:
        Y = DiehlAndCookNodes(n=N, traces=True, theta_plus=0.05, tc_theta_decay=1e7)
        conn = MulticompartmentConnection(X, Y, device="cpu", pipeline=[
            Weight("weight", w, range=[lo, hi], norm=norm, nu=[1e-4, 1e-2], reduction=torch.sum, learning_rule=MccPostPre)])
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(conn, "X", "Y")
    return net.to("cuda:0")


def weights(net):
    conn = net.connections[("X", "Y")]
    return conn.pipeline[0].value if hasattr(conn, "pipeline") else conn.w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--graphs", nargs="+", default=["dense", "mcc"], choices=sorted(GRAPHS))
    ap.add_argument("--modes", nargs="+", default=["scalar", "uniform", "tensor"], choices=["scalar", "uniform", "tensor"])
    a = ap.parse_args()
    from bindsnet_amd import _lib
    _lib.lib().snn_set_plan_mode(1)                    # the generic plan for the scalar rows as well
    for graph in a.graphs:
        B = GRAPHS[graph]["B"]
        x = torch.from_numpy((np.random.default_rng(2).random((a.time, B, S)) < 0.1).astype(np.uint8)).to("cuda:0")
        medians = {}
        for mode in a.modes:
            net = build(graph, mode)
            theta = getattr(net.layers["Y"], "theta", None)
            w, w0 = weights(net), weights(net).detach().clone()
            torch.manual_seed(3)
            net.run({"X": x}, time=a.time)
            net.reset_state_variables()
            torch.cuda.synchronize()
            rates = []
            for _ in range(a.repeats):
                w.data.copy_(w0)
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
            print(json.dumps({"graph": graph, "mode": mode, "plan": net.last_plan, "S": S, "N": N, "B": B, "T": a.time,
                              "runs_per_repeat": a.runs, "timesteps_per_s": [round(r, 1) for r in rates],
                              "median": round(medians[mode], 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}), flush=True)
        if "scalar" in medians and len(medians) > 1:
            print(json.dumps({"graph": graph, **{f"{m}_over_scalar": round(v / medians["scalar"], 4) for m, v in medians.items() if m != "scalar"}}),
                  flush=True)


if __name__ == "__main__":
    main()
