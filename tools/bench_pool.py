#!/usr/bin/env python3
"""Timesteps/s of a small convolutional SNN with pooling and global inhibition -- Input 1x28x28 -> Conv2dConnection (16 filters 5x5,
PostPre) -> LIFNodes (16, 24, 24) -> MaxPool2dConnection(2, 2) -> LIFNodes (16, 12, 12), with a recurrent MeanFieldConnection
(w = -2) on the pooled layer, T = 250, network.train(True) -- on the MI355X (generic plan) and on the host path, same commit.

    python tools/bench_pool.py [--time 250] [--runs 100] [--batch 1 16] [--host-runs 5] [--meanfield]

Points: batch in {1, 16}; Bernoulli input at 10 %.  Per point and side: one untimed run, then `runs` network.run(time) calls, each
followed by reset_state_variables(), timed end to end (the device synchronised); the defaults make every timed window last about a
second or more, and each line carries its window's length.  The weights are drawn once per point and restored
before every side's runs, so both sides do the same work.  Prints one JSON line per point: timesteps/s of both sides, the pooled
layer's spikes per step and sample, and whether the device's raster of the pooled layer equals the host path's (it must: every
connection of the graph is bit-exact on the generic plan).

--meanfield: instead, the time of one snn_prop_meanfield_f32 call (device events around 20 calls, after 3 untimed ones) for source
tensors of 2^12 .. 2^24 spike bytes and 2^20 targets: every one of its 64 workgroups counts the whole source tensor."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
DEV = "cuda:0"


def network(B, w0):
    from bindsnet_amd.learning import PostPre
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Conv2dConnection, MaxPool2dConnection, MeanFieldConnection
    net = Network(dt=1.0, batch_size=B)
    X, C, P = Input(shape=(1, 28, 28), traces=True), LIFNodes(shape=(16, 24, 24), traces=True, thresh=-62.0), \
        LIFNodes(shape=(16, 12, 12), traces=True, thresh=-63.0)
    for name, layer in (("X", X), ("C", C), ("P", P)):
        net.add_layer(layer, name)
    net.add_connection(Conv2dConnection(X, C, kernel_size=5, stride=1, update_rule=PostPre, nu=(1e-4, 1e-3), reduction=torch.sum,
                                        wmin=0.0, wmax=1.0, w=w0.clone()), "X", "C")
    net.add_connection(MaxPool2dConnection(C, P, kernel_size=2, stride=2, decay=0.2), "C", "P")
    net.add_connection(MeanFieldConnection(P, P, w=torch.tensor(-2.0)), "P", "P")
    net.train(True)
    return net


def timed(net, x, T, runs, sync):
    from bindsnet_amd.network.monitors import Monitor
    mon = Monitor(net.layers["P"], ["s"], time=T)
    net.add_monitor(mon, "P")
    net.run({"X": x.clone()}, time=T)                          # untimed; also what the rasters are compared on
    raster = mon.get("s").clone().cpu()
    del net.monitors["P"]
    net.reset_state_variables()
    sync()
    t0 = time.perf_counter()
    for _ in range(runs):
        net.run({"X": x.clone()}, time=T)
        net.reset_state_variables()
    sync()
    window = time.perf_counter() - t0
    return runs * T / window, raster, window


def meanfield_calls():
    from bindsnet_amd import ops
    n_tgt = 1 << 20
    w, out = torch.tensor(-0.5, device=DEV), torch.zeros(1, n_tgt, device=DEV)
    for log2 in (12, 16, 20, 22, 24):
        s = (torch.rand(1, 1 << log2, device=DEV) < 0.1).to(torch.uint8)
        for _ in range(3):
            ops.prop_meanfield(w, s, out)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(20):
            ops.prop_meanfield(w, s, out)
        end.record()
        torch.cuda.synchronize()
        print(json.dumps({"op": "prop_meanfield", "source_bytes": 1 << log2, "targets": n_tgt, "calls": 20,
                          "us_per_call": round(1000.0 * start.elapsed_time(end) / 20, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--meanfield", action="store_true")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pool.py measures on the MI355X: no GPU here")
    if a.meanfield:
        return meanfield_calls()
    for B in a.batch:
        g = torch.Generator().manual_seed(B)
        x = (torch.rand(a.time, B, 1, 28, 28, generator=g) < 0.1).to(torch.uint8)
        w0 = torch.rand(16, 1, 5, 5, generator=g)
        line = {"graph": "Input 1x28x28 -> Conv2d 16x5x5 PostPre -> LIF -> MaxPool2d(2,2) -> LIF + MeanField", "B": B, "T": a.time}
        rasters = {}
        for side in ("device", "host"):
            net = network(B, w0)
            if side == "device":
                net = net.to(DEV)
            runs = a.runs if side == "device" else a.host_runs
            rate, rasters[side], window = timed(net, x.to(DEV) if side == "device" else x, a.time, runs,
                                        torch.cuda.synchronize if side == "device" else (lambda: None))
            line[side + "_timesteps_per_s"], line[side + "_us_per_timestep"] = round(rate, 1), round(1e6 / rate, 2)
            line[side + "_runs"], line[side + "_window_s"], line[side + "_plan"] = runs, round(window, 3), net.last_plan
        line["pooled_spikes_per_step_and_sample"] = round(float(rasters["device"].sum()) / (a.time * B), 2)
        line["raster_equals_host"] = bool(torch.equal(rasters["device"], rasters["host"]))
        line["device_over_host"] = round(line["device_timesteps_per_s"] / line["host_timesteps_per_s"], 2)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
