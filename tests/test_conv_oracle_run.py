"""tests/conv_oracle_run.py -- the stepped CPU-oracle run the conv plans are checked against (tests/test_gpu_conv_oracle.py) -- pinned to the
reference: the run_extras "crun" run (tests/golden/make_golden_r2.py; test_gpu_extras.py checks both device plans against the same fixture)
rebuilt through the helper.  Input(1,12,12) -> Conv2dConnection 3x3x4 [PostPre] -> LIFNodes(4,10,10), batch 2, 30 steps."""
import numpy as np
import torch

import synth
from cases import gold, u8, unpack
from conv_oracle_run import ConvOracleRun


def crun_network():
    from bindsnet_amd.learning import PostPre
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import Conv2dConnection
    net = Network(dt=1.0)
    net.add_layer(Input(shape=(1, 12, 12), traces=True), "X")
    net.add_layer(LIFNodes(shape=(4, 10, 10), traces=True), "Y")
    cc = Conv2dConnection(net.layers["X"], net.layers["Y"], kernel_size=3, stride=1, w=torch.from_numpy(synth.uniform_f32(1700, (4, 1, 3, 3), 0.0, 3.0)),
                          update_rule=PostPre, nu=(1e-3, 1e-2), reduction=torch.sum, wmin=0.0, wmax=4.0)
    net.add_connection(cc, "X", "Y")
    return net


def test_stepped_conv_postpre_run_matches_reference_crun():
    g = gold("run_extras")
    B, T = 2, 30
    orc = ConvOracleRun(crun_network(), B)
    out = orc.run(synth.dense_spikes(1701, (T, B, 1, 12, 12), 0.2))
    np.testing.assert_array_equal(out["s"].reshape(T, B, 400), unpack(g["crun_sY"], (T, B, 400)))
    # the reference sums over batch and positions inside torch.bmm (BLAS order): 30 updates accumulate that, relative to wmax = 4.0
    np.testing.assert_allclose(out["W"], g["crun_W"], rtol=0, atol=1e-5 * 4.0)
    assert out["s"].sum() > 100
    assert not np.array_equal(out["W"], synth.uniform_f32(1700, (4, 1, 3, 3), 0.0, 3.0))


def test_state_carries_across_runs():
    """Two runs of 15 steps give the bits of one run of 30: the second run's first convolution reads the first run's last input spikes."""
    B, T = 2, 30
    sp = synth.dense_spikes(1701, (T, B, 1, 12, 12), 0.2)
    whole = ConvOracleRun(crun_network(), B).run(sp, voltages=True)
    orc = ConvOracleRun(crun_network(), B)
    first, second = orc.run(sp[:15], voltages=True), orc.run(sp[15:], voltages=True)
    np.testing.assert_array_equal(np.concatenate([first["s"], second["s"]]), whole["s"])
    np.testing.assert_array_equal(np.concatenate([first["vras"], second["vras"]]).view(np.uint32), whole["vras"].view(np.uint32))
    for k in ("v", "refrac_count", "sY", "xY", "xX", "W"):
        np.testing.assert_array_equal(second[k].view(u8), whole[k].view(u8), err_msg=k)
