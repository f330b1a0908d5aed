"""bench.py's headline command end to end on the MI355X: a plain run times its steps and prints the line without the secondary legs;
`--dump-outputs` writes what the last timed step computed; `--full` adds the secondary legs and leaves the timed steps' results as they were."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, W = 3, 2
SECONDARY = ("cpu_baseline", "parity", "sync_runs", "roofline")


def _bench(args, timeout=400):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W)] + args,
                         capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert res.returncode == 0 and lines, (res.stdout[-1500:], res.stderr[-3000:])
    return json.loads(lines[-1])


def _load(d):
    return {f[:-len(".npy")]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    return _bench(["--dump-outputs", str(d)]), _load(d)


def test_plain_run_line(plain):
    line, _ = plain
    assert line["steps"] == K and line["warmup"] == W and line["unit"] == "timesteps/s" and line["higher_is_better"] and line["dtype"] == "f32"
    assert abs(line["value"] - 250 * 1e3 / line["ms_per_step"]) / line["value"] < 1e-3
    assert line["config"]["plan"].startswith("dc2015-resident")
    assert all(line[k] is None for k in SECONDARY)


def test_dump_outputs_hold_the_last_timed_step(plain):
    _, out = plain
    assert sorted(out) == ["Ae_spikes", "Ai_spikes", "W_X_Ae", "X_spikes", "theta_Ae"]
    assert all(a.dtype == np.float32 for a in out.values()) and sum(a.nbytes for a in out.values()) <= 64 << 20
    assert out["Ae_spikes"].shape == out["Ai_spikes"].shape == (250, 32, 400) and out["W_X_Ae"].shape == (784, 400)
    assert out["theta_Ae"].shape == (400,) and out["theta_Ae"].max() > 0
    for k in ("Ae_spikes", "Ai_spikes"):
        assert set(np.unique(out[k])) <= {0.0, 1.0} and out[k].sum() > 0
    # the X monitor records the input the last timed step ran on: batch (W + K - 1) % 4 of bench.py's seeded pool
    from bindsnet_amd import synth
    x = synth.poisson_mnist_like(32, 250, 4, seed=1)[(W + K - 1) % 4]
    np.testing.assert_array_equal(out["X_spikes"].reshape(250, 32, 784), x.reshape(250, 32, 784).astype(np.float32))


def test_full_adds_the_secondary_legs_and_computes_the_same(plain, tmp_path):
    line = _bench(["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)])
    assert line["sync_runs"]["steps"] == K and line["roofline"]["launches_timed"] > 0
    out = _load(tmp_path)
    for k, a in plain[1].items():
        np.testing.assert_array_equal(out[k], a, err_msg=k)
