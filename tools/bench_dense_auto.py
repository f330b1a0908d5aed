#!/usr/bin/env python3
"""Connection.compute with its body chosen on the device (snn_prop_dense_auto_f32) on one MI355X, against the two kernels it chooses
between, and the networks that run it.  profiles/NOTES_dense_auto.md has the windows this printed and the constants of
csrc/snn_dense_auto.hpp that were fitted to them.

    python tools/bench_dense_auto.py op  [--iters 200] [--reps 5]
    python tools/bench_dense_auto.py net [--time 100] [--runs 10] [--reps 5] [--against PARENT_CHECKOUT [--rounds 2]]

op:  per shape and input density, microseconds per call of `event` (ops.prop_dense), `matrix` (ops.prop_dense_mfma), `auto` (the cost
     rule), `auto_event` and `auto_matrix` (the auto entry point forced to one body: what the rule really chooses between), and of
     `boundary`, an empty-handed launch (one thread) -- 10 untimed calls, then `reps` windows of `iters` calls between device events,
     the forms taking turns window by window; the median with [min, max].  `tiles` says which body `auto` took.
net: timesteps per second of the converted MLP of tools/bench_analog.py on its uint8 Poisson train and of the breakout graph of
     tools/bench_nodes.py (LIF layers) on Bernoulli input at 1 % and at 30 % -- as built and, where the checkout knows it, with
     prop_auto=True on its connections --, and of a sparse 784 -> 400 -> 100 graph of plain Connections, batch 1 and 16: one untimed run, then `reps` windows of
     `runs` runs, each followed by reset_state_variables(), timed end to end with the device synchronised.  With --against the same
     rows are taken from another checkout of the package (built there) in processes of their own, the two taking turns `rounds`
     times; every process prints its windows and, where the checkout has them, the prop_stats() of a run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if "--root" in sys.argv:                        # (net: the checkout whose package is measured)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

DEV = "cuda:0"
SHAPES = [(16, 784, 1600), (32, 784, 1600), (128, 784, 1600), (16, 6400, 500),          # those of tools/bench_dense_prop.py
          (1, 784, 256), (16, 784, 256), (16, 256, 128), (1, 6400, 100), (16, 6400, 100)]
DENSITIES = (0.01, 0.03, 0.05, 0.08, 0.12, 0.20, 0.50)


def med(xs, nd=2):
    return [round(statistics.median(xs), nd), round(min(xs), nd), round(max(xs), nd)]


def op(a):
    import torch
    from bindsnet_amd import ops, synth
    one, one_out, nil = torch.zeros(1, 1, device=DEV), torch.zeros(1, 1, device=DEV), torch.zeros(1, 1, dtype=torch.uint8, device=DEV)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    for B, Nin, N in SHAPES:
        W = torch.from_numpy(synth.uniform_f32(1, (Nin, N), 0.0, 0.3)).to(DEV)
        out = torch.empty(B, N, device=DEV)
        flags = torch.empty((B + 15) // 16, dtype=torch.int32, device=DEV)
        for dens in DENSITIES:
            s = torch.from_numpy(synth.dense_spikes(2, (B, Nin), dens)).to(DEV)
            cnt = torch.zeros(2, dtype=torch.int32, device=DEV)

            def auto(mode):
                def fn():
                    ops.prop_dense_auto(W, s, out, counters=cnt, flags=flags)
                return mode, fn
            forms = {"event": (0, lambda: ops.prop_dense(W, s, out)), "matrix": (0, lambda: ops.prop_dense_mfma(W, s, out)),
                     "auto": auto(0), "auto_event": auto(1), "auto_matrix": auto(2),
                     "boundary": (0, lambda: ops.prop_dense(one, nil, one_out))}       # one workgroup, no event: a launch and nothing else
            times = {k: [] for k in forms}
            for k, (mode, fn) in forms.items():
                ops.set_dense_prop_mode(mode)
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            cnt.zero_()
            for _ in range(a.reps):
                for k, (mode, fn) in forms.items():
                    ops.set_dense_prop_mode(mode)
                    if k == "auto":
                        before = cnt.tolist()
                    times[k].append(window(fn))
                    if k == "auto":
                        after = cnt.tolist()
            ops.set_dense_prop_mode(0)
            line = {"B": B, "Nin": Nin, "N": N, "density": dens, "max_events": int((s != 0).sum(1).max())}
            line.update({k + "_us": med(v) for k, v in times.items()})
            line["tiles"] = {"matrix": after[0] - before[0], "event": after[1] - before[1]}
            best = min(line["event_us"][0], line["matrix_us"][0])
            spread = max(v[2] - v[1] for v in (line["auto_us"], line["event_us"], line["matrix_us"]))
            line["auto_over_best_us"] = round(line["auto_us"][0] - best, 2)
            line["allowance_us"] = round(line["boundary_us"][0] + spread, 2)
            line["within"] = line["auto_over_best_us"] <= line["allowance_us"]
            print(json.dumps(line), flush=True)


def net_rows(a):
    import warnings
    import torch
    import bench_analog
    import node_cases as NC
    from bindsnet_amd.learning import learning
    from bindsnet_amd.network import Network, nodes, topology

    def measure(label, B, net, inputs, kw):
        net.run(inputs(), time=a.time, **kw)
        stats = net.prop_stats() if hasattr(net, "prop_stats") else None
        net.reset_state_variables()
        rates = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.runs):
                net.run(inputs(), time=a.time, **kw)
                net.reset_state_variables()
            torch.cuda.synchronize()
            rates.append(a.runs * a.time / (time.perf_counter() - t0))
        line = {"tree": a.tag, "graph": label, "B": B, "T": a.time, "runs_per_window": a.runs, "plan": net.last_plan,
                "timesteps_per_s": med(rates, 1), "windows": [round(r, 1) for r in rates]}
        if stats is not None:
            line["prop_stats_of_one_run"] = {"->".join(k): v for k, v in stats.items()}
        print(json.dumps(line), flush=True)

    for B in (1, 16):
        img = bench_analog.image("mlp", B)
        x = (torch.rand(a.time, *img.shape, generator=torch.Generator().manual_seed(100 + B)) < img).to(torch.uint8).to(DEV)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            net = bench_analog.network("mlp", B).to(DEV)
        measure("ann_to_snn MLP 784-256-128-10, uint8 Poisson train", B, net, lambda: {"Input": x.clone()}, {})
    can_ask = hasattr(topology.Connection(nodes.Input(n=1), nodes.LIFNodes(n=1), w=torch.zeros(1, 1)), "prop_auto")
    for p in (0.01, 0.30):
        for B in (1, 16):
            for ask in (False, True) if can_ask else (False,):
                net = NC.breakout_graph(nodes, topology, learning, Network, "lif")
                if ask:
                    for c in net.connections.values():
                        c.prop_auto = True
                net = net.to(DEV)
                x = torch.from_numpy(NC.breakout_input(a.time, B, p=p)).to(DEV)
                measure(f"breakout shape 6400 -> 100 -> 4 (LIF, MSTDP), Bernoulli {p:.0%}" + (", prop_auto=True" if ask else ""), B, net,
                        lambda: {"X": x}, {"reward": 1.0})
    for B in (1, 16):       # a sparse graph of plain Connections with 784 sources: Input 784 -> LIF 400 -> LIF 100, 1 % Bernoulli input
        g = torch.Generator().manual_seed(7)
        net = Network(dt=1.0)
        for name, layer in (("X", nodes.Input(n=784, traces=True)), ("H", nodes.LIFNodes(n=400, traces=True)), ("Y", nodes.LIFNodes(n=100, traces=True))):
            net.add_layer(layer, name)
        net.add_connection(topology.Connection(net.layers["X"], net.layers["H"], w=torch.rand(784, 400, generator=g) * 0.6), "X", "H")
        net.add_connection(topology.Connection(net.layers["H"], net.layers["Y"], w=torch.rand(400, 100, generator=g) * 0.3), "H", "Y")
        net = net.to(DEV)
        x = (torch.rand(a.time, B, 784, generator=torch.Generator().manual_seed(B)) < 0.01).to(torch.uint8).to(DEV)
        measure("Input 784 -> LIF 400 -> LIF 100, plain Connections, Bernoulli 1%", B, net, lambda: {"X": x}, {})


def net(a):
    if not a.against:
        return net_rows(a)
    trees = (("this", ROOT), ("parent", os.path.abspath(a.against)))
    for rnd in range(a.rounds):
        for tag, root in trees:
            cmd = [sys.executable, os.path.abspath(__file__), "net", "--root", root, "--tag", f"{tag} (round {rnd})", "--time", str(a.time),
                   "--runs", str(a.runs), "--reps", str(a.reps)]
            subprocess.run(cmd, check=True, cwd=root, timeout=a.child_timeout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["op", "net"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--time", type=int, default=100)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--against", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--tag", default="this")
    a = ap.parse_args()
    {"op": op, "net": net}[a.what](a)


if __name__ == "__main__":
    main()
