"""The EXACT batch-sharded mode (bindsnet_amd.parallel.exact_run: one all-gather of the spikes per timestep, the coupled
operations -- theta bump, one_spike draws in global row order, PostPre's batch sum -- on the global batch, identically on
every rank) ON THE DEVICE: the C ABI's per-operator entry points incl. snn_dc_arbitrate (ABI 5), against what the unmodified
reference computed for the GLOBAL batch in one process.  tests/test_parallel_gloo.py runs the same schedule on the host
operators at world 2 / 3 / 4.  (The file sorts last on purpose: these tests start extra processes that share the GPU.)"""
import pytest

pytestmark = pytest.mark.gpu


def test_exact_mode_single_rank_on_the_gpu(tmp_path):
    """World size 1 (no process group): exact_run's operator sequence alone == the reference fixture, bit for bit."""
    import exact_harness as H
    res = H.launch(1, "run_dc_n400_b4", "cuda", tmp_path, timeout=240)
    H.check_against_reference(res, "run_dc_n400_b4")


def test_exact_mode_two_ranks_on_one_gpu(tmp_path):
    """Two processes on the one GPU (gloo between them), 16 + 16 rows of BASELINE cfg2's stated input, three consecutive
    inputs: rows side by side == the reference's single-process global batch of 32 -- rasters, weights, theta, membrane
    state, traces bit for bit, and both host generators where the reference's stands."""
    import exact_harness as H
    name = "full_cfg2_dc_n400_b32_poisson"
    res = H.launch(2, name, "cuda", tmp_path, timeout=240)
    H.check_against_reference(res, name)


def test_exact_gathered_mode_two_ranks_on_one_gpu_runs_the_resident_kernel(tmp_path):
    """exact_run(mode="auto") at a global batch of 32: one all-gather of the inputs and the state per run, then BOTH ranks run the global batch
    through the resident D&C kernel (one launch per run) and keep their 16 rows -- == the reference's single-process global batch of
    BASELINE cfg2's stated input (three consecutive inputs: rasters, weights, theta, membrane state, traces, generator position), at the
    single-GPU kernel's speed instead of the per-step schedule's 2.3 k timesteps/s (round 5).
    Skipped where the device grants cooperative launches -- the resident kernel's -- to one process at a time."""
    import coop_probe
    reason = coop_probe.refusal()
    if reason:
        pytest.skip(reason)
    import exact_harness as H
    name = "full_cfg2_dc_n400_b32_poisson"
    res = H.launch(2, name, "cuda", tmp_path, timeout=240, mode="auto")
    H.check_against_reference(res, name)
    for r in res:
        assert str(r["r0_plan"]).startswith("exact-gathered:dc2015-resident"), str(r["r0_plan"])
    # the rank that reaches the run's one collective LAST measures what a run costs (the other one's time contains its wait for the peer, whose
    # worker packs and stores its outputs between the runs); two processes share the one GPU here, each running the whole batch
    rate = 250 / min(float(r["r2_seconds"]) for r in res)
    print(f"exact_run gathered, two ranks on one GPU: {rate:.0f} timesteps/s")     # (53 k alone on the box, profiles/r06_exact_gathered_phase_timing.log;
    assert rate > 1000, f"{rate:.0f} timesteps/s"                                  #  no tight bound in the test tier: the two processes time-share the GPU)
