"""Do two processes on one device both get cooperative launches?  The resident D&C plan is one cooperative launch per run, and a device that
processes share may grant its cooperative queue to one of them only: every other process then runs the one-launch-per-timestep plan (same
numbers, other plan name).  Tests that need the resident plan in SEVERAL processes at once ask here first, once per session: this process
runs a tiny D&C network (and so holds the queue, if it can be had), then a child process does the same and tells its plan."""
import functools
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def tiny_run():
    """The plan of one run of a 784 -> 64 D&C network, batch 2, 8 timesteps, on the device."""
    import torch
    from bindsnet_amd.models import DiehlAndCook2015
    net = DiehlAndCook2015(n_inpt=784, n_neurons=64, exc=22.5, inh=120, dt=1.0, norm=78.4, theta_plus=0.05, inpt_shape=(1, 28, 28))
    net.to("cuda")
    net.run({"X": torch.zeros(8, 2, 1, 28, 28, dtype=torch.uint8, device="cuda")}, time=8)
    torch.cuda.synchronize()
    return net.last_plan


@functools.lru_cache(maxsize=None)
def refusal():
    """None where a second process gets the resident plan beside this one; else the reason to give pytest.skip."""
    own = tiny_run()
    code = "import sys; sys.path[:0] = [%r, %r]; import coop_probe; print('plan', coop_probe.tiny_run())" % (ROOT, HERE)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    plans = [l.split()[1] for l in out.stdout.splitlines() if l.startswith("plan ")]
    if out.returncode != 0 or not plans:
        return None                                        # the probe itself broke: let the test run and show why
    if own.startswith("dc2015-resident") and plans[0].startswith("dc2015-resident"):
        return None
    return ("cooperative launches by more than one process at a time are not supported here: "
            f"the resident plan ran as {own} in this process and as {plans[0]} in a second one")
