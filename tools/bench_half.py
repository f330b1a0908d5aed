#!/usr/bin/env python3
"""Timesteps/s of DiehlAndCook2015 784 -> 400, batch 32, T = 250, PostPre on, on one MI355X, by the dtype of its Weight features:

    f32_generic   float32 with the generic plan forced (snn_set_plan_mode(1)): the like-for-like baseline of the half runs
    f16, bf16     w_dtype=torch.float16 / torch.bfloat16: on the generic plan by construction (csrc/snn_half.hip)
    f32_resident  float32 on the plan the library picks (the resident kernel), for scale

    python tools/bench_half.py [--windows 7] [--runs 4] [--warmup 2] [--time 250] [--batch 32] [--neurons 400]

Method: the four networks are built from the same seed and see the same Bernoulli input (density 0.12).  Each takes `warmup` untimed
runs; then `windows` rounds visit the variants in turn (alternating, so drift hits all alike), and a window is `runs` calls of
network.run(time) + reset_state_variables() between two device synchronisations, on the host clock.  Prints one JSON line: per
variant the plan, the median timesteps/s over the windows, the spread (min, max) and us per timestep, and each half variant's median
over f32_generic's.  Whether the variants computed something sensible is the tests' business (tests/test_gpu_half.py), not this
tool's; it only reports the Ae spike count of the last warm-up run."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
DEV = "cuda:0"
VARIANTS = {"f32_generic": (torch.float32, 1), "f16": (torch.float16, 0), "bf16": (torch.bfloat16, 0), "f32_resident": (torch.float32, 0)}


def build(dtype, n, B):
    from bindsnet_amd.models import DiehlAndCook2015
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        net = DiehlAndCook2015(n_inpt=784, n_neurons=n, batch_size=B, exc=22.5, inh=120, dt=1.0, norm=78.4, nu=(1e-4, 1e-2), theta_plus=0.05,
                               inpt_shape=(1, 28, 28), w_dtype=dtype)
    return net.to(DEV)


def window(net, x, T, runs, mode, lib):
    lib.snn_set_plan_mode(mode)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        net.run({"X": x.clone()}, time=T)      # (a clone: Input.s aliases the last slice, which the reset clears)
        net.reset_state_variables()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lib.snn_set_plan_mode(0)
    return runs * T / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--time", type=int, default=250)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--neurons", type=int, default=400)
    a = ap.parse_args()
    if a.windows < 5:
        raise SystemExit("bench_half.py: at least 5 timed windows")
    if not torch.cuda.is_available():
        raise SystemExit("bench_half.py measures on the MI355X: no GPU here")
    from bindsnet_amd import _lib
    from bindsnet_amd.network.monitors import Monitor
    lib = _lib.lib()
    x = torch.from_numpy((np.random.default_rng(0).random((a.time, a.batch, 1, 28, 28)) < 0.12).astype(np.uint8)).to(DEV)
    nets, line = {}, {"graph": f"DiehlAndCook2015 784 -> {a.neurons}", "B": a.batch, "T": a.time, "windows": a.windows, "runs_per_window": a.runs,
                      "variants": {}}
    for name, (dtype, mode) in VARIANTS.items():
        net = nets[name] = build(dtype, a.neurons, a.batch)
        mon = Monitor(net.layers["Ae"], ["s"], time=a.time)
        net.add_monitor(mon, "Ae_s")
        lib.snn_set_plan_mode(mode)
        for _ in range(max(1, a.warmup)):
            net.run({"X": x.clone()}, time=a.time)
            spikes = int(mon.get("s").sum())
            net.reset_state_variables()
        lib.snn_set_plan_mode(0)
        del net.monitors["Ae_s"]
        line["variants"][name] = {"plan": net.last_plan, "ae_spikes_last_warmup": spikes, "rates": []}
    for _ in range(a.windows):
        for name, (dtype, mode) in VARIANTS.items():
            line["variants"][name]["rates"].append(window(nets[name], x, a.time, a.runs, mode, lib))
    for name, v in line["variants"].items():
        rates = v.pop("rates")
        med = statistics.median(rates)
        v.update(timesteps_per_s_median=round(med, 1), timesteps_per_s_min=round(min(rates), 1), timesteps_per_s_max=round(max(rates), 1),
                 us_per_timestep_median=round(1e6 / med, 2), spread_pct=round(100.0 * (max(rates) - min(rates)) / med, 1))
    base = line["variants"]["f32_generic"]["timesteps_per_s_median"]
    for name in ("f16", "bf16", "f32_resident"):
        line["variants"][name]["over_f32_generic"] = round(line["variants"][name]["timesteps_per_s_median"] / base, 3)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
