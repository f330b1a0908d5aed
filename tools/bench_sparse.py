#!/usr/bin/env python3
"""Timesteps/s of a sparse reservoir -- Input 784 -> SparseConnection -> LIFNodes(n), with a recurrent SparseConnection n -> n, T = 250
-- on the MI355X (generic plan), once with the two SparseConnections and once with the SAME weights densified into two
Connections, on the same commit.  The dense Connection is the only other way this package runs the graph, so it is the baseline.

    python tools/bench_sparse.py [--time 250] [--runs 3] [--n 4096 16384] [--density 0.01 0.05] [--batch 1 16]

Points: n in {4096, 16384}, weight density in {1 %, 5 %}, batch in {1, 16}; Bernoulli input at 1.2 %.  The input
weights are positive and scaled so that the input alone drives a neuron to about 1.5 times its threshold distance; the recurrent
weights are uniform in [-0.5, 0.5).  Per point and form: one untimed run, then `runs` network.run(time) calls, each followed by
reset_state_variables(), timed end to end with the device synchronised.  Prints one JSON line per point: timesteps/s of both forms,
the reservoir's spikes per step and sample, whether both forms gave the same raster (they must: both sum in ascending source
order), and the device bytes the weights hold -- the compiled form (ptr + col + val) plus the COO tensor `w` itself against the two
dense matrices."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
DEV = "cuda:0"


def weights(n_in, n, density, seed):
    """(input matrix [n_in, n], recurrent matrix [n, n]) as dense device tensors; exact zeros are the absent synapses."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    drive = 20.0 / (100.0 * 0.012 * n_in * density)            # mean input weight: steady-state input of about 20 mV
    w_in = 2.0 * drive * torch.rand(n_in, n, device=DEV, generator=g) * (torch.rand(n_in, n, device=DEV, generator=g) < density)
    w_rec = torch.rand(n, n, device=DEV, generator=g)
    w_rec.sub_(0.5).mul_(torch.rand(n, n, device=DEV, generator=g) < density)
    return w_in, w_rec


def reservoir(w_in, w_rec, sparse):
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Connection, SparseConnection
    cls = SparseConnection if sparse else Connection
    net = Network(dt=1.0)
    X, Y = Input(n=w_in.shape[0]), LIFNodes(n=w_in.shape[1])
    net.add_layer(X, "X")
    net.add_layer(Y, "Y")
    net.add_connection(cls(X, Y, w=w_in), "X", "Y")
    net.add_connection(cls(Y, Y, w=w_rec), "Y", "Y")
    return net.to(DEV)


def held_bytes(net, sparse):
    total = 0
    for conn in net.connections.values():
        if sparse:
            total += sum(t.numel() * t.element_size() for t in conn._compiled())
            total += sum(t.numel() * t.element_size() for t in (conn.w._indices(), conn.w._values()))
        else:
            total += conn.w.numel() * conn.w.element_size()
    return total


def timed(net, x, T, runs):
    from bindsnet_amd.network.monitors import Monitor
    mon = Monitor(net.layers["Y"], ["s"], time=T)
    net.add_monitor(mon, "Y")
    net.run({"X": x.clone()}, time=T)                          # untimed; also what the rasters are compared on (a clone: Input.s
                                                               # aliases the last slice, which reset_state_variables() clears)
    raster = mon.get("s").clone()
    del net.monitors["Y"]
    net.reset_state_variables()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        net.run({"X": x.clone()}, time=T)
        net.reset_state_variables()
    torch.cuda.synchronize()
    return runs * T / (time.perf_counter() - t0), raster


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--density", type=float, nargs="+", default=[0.01, 0.05])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse.py measures on the MI355X: no GPU here")
    for n in a.n:
        for density in a.density:
            w_in, w_rec = weights(784, n, density, seed=n + int(1000 * density))
            for B in a.batch:
                g = torch.Generator(device=DEV).manual_seed(B)
                x = (torch.rand(a.time, B, 784, device=DEV, generator=g) < 0.012).to(torch.uint8)
                line = {"graph": "Input 784 -> LIF n + recurrent n -> n", "n": n, "density": density, "B": B, "T": a.time, "runs": a.runs}
                rasters = {}
                for form in ("sparse", "dense"):
                    net = reservoir(w_in, w_rec, form == "sparse")
                    rate, rasters[form] = timed(net, x, a.time, a.runs)
                    line[form + "_timesteps_per_s"] = round(rate, 1)
                    line[form + "_us_per_timestep"] = round(1e6 / rate, 2)
                    line[form + "_weight_bytes"] = held_bytes(net, form == "sparse")
                    line["plan"] = net.last_plan
                    if form == "sparse":
                        line["nnz"] = [int(c.w._nnz()) for c in net.connections.values()]
                    del net
                    torch.cuda.empty_cache()
                line["spikes_per_step_and_sample"] = round(float(rasters["sparse"].sum()) / (a.time * B), 2)
                line["raster_equals_dense"] = bool(torch.equal(rasters["sparse"], rasters["dense"]))
                line["sparse_over_dense"] = round(line["sparse_timesteps_per_s"] / line["dense_timesteps_per_s"], 3)
                print(json.dumps(line), flush=True)
            del w_in, w_rec
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
