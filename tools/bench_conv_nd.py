#!/usr/bin/env python3
"""Timesteps/s of the conv1d_MNIST.py and conv3d_MNIST.py graphs (tests/conv_nd_cases.py cases (a) and (d), the latter with
conv3d_MNIST.py's 25 filters: Conv1dConnection
k 56 s 28, 25 filters, PostPre, and Conv3dConnection k 16 s 4 on a 28^3 input with PostPre nu = (0, 1e-2) -- the only
conv3d learning the reference defines -- each into DiehlAndCookNodes with the recurrent inhibition) on the MI355X, generic
plan, learning on; and, in the same command, the package's own host path (plain PyTorch) on the same graphs.

    python tools/bench_conv_nd.py [--time 250] [--runs 5] [--host-runs 1]    (--host-runs 0: the device only)

Per case: one untimed run, then `runs` network.run(time) calls on random input (5 % dense for conv1d, a 3 % dense plane
repeated along depth for conv3d), each followed by reset_state_variables(), timed end to end with the device synchronised.
Prints one JSON line per (case, path)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

GRAPHS = [("conv1d", "a", 1), ("conv1d", "a", 32), ("conv3d", "d25", 1)]


def _input(name, B, T, seed):
    import conv_nd_cases as CC
    c = CC.CASES[name]
    rng = np.random.default_rng(seed)
    if c["kind"] == "c3":
        plane = (rng.random((T, B, 1, 1, 28, 28)) < c["density"]).astype(np.uint8)
        return torch.from_numpy(np.ascontiguousarray(np.repeat(plane, 28, axis=3)))
    return torch.from_numpy((rng.random((T, B, 1, 784)) < c["density"]).astype(np.uint8))


def _time(net, x, T, runs, sync):
    net.run({"X": x}, time=T)
    net.reset_state_variables()
    sync()
    t0 = time.perf_counter()
    for _ in range(runs):
        net.run({"X": x}, time=T)
        net.reset_state_variables()
    sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=1)
    a = ap.parse_args()
    import conv_nd_cases as CC
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network, nodes, topology
    ns = CC.ns_from(nodes, topology, learning, Network)
    CC.CASES["d25"] = dict(CC.CASES["d"], F=25)          # conv3d_MNIST.py's 25 filters (the fixture keeps 12)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for graph, name, B in GRAPHS:
        for path, dev, runs in (("device", "cuda:0", a.runs), ("host", "cpu", a.host_runs)):
            if runs <= 0:
                continue
            net = CC.build(ns, name).to(dev)
            x = _input(name, B, a.time, B).to(dev)
            sync = torch.cuda.synchronize if dev != "cpu" else (lambda: None)
            dt = _time(net, x, a.time, runs, sync)
            print(json.dumps({"graph": f"{graph} ({'Conv1d' if graph == 'conv1d' else 'Conv3d'}Connection PostPre + D&C + "
                                       "recurrent inhibition)", "path": path, "plan": net.last_plan, "B": B, "T": a.time,
                              "filters": CC.CASES[name]["F"], "runs": runs, "timesteps_per_s": round(runs * a.time / dt, 1),
                              "us_per_timestep": round(1e6 * dt / (runs * a.time), 2), "ms_per_run": round(1e3 * dt / runs, 3)}),
                  flush=True)


if __name__ == "__main__":
    main()
