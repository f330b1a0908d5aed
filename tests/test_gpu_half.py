"""float16 / bfloat16 Weight features on the MI355X (csrc/snn_half.hip, the generic plan of snn_net_run).  Every comparison is on raw bits.

  * every fixture case of tests/half_cases.py (the unmodified reference, tests/golden/make_golden_half.py) on the device: rasters, neuron
    state, traces, the learned value's 16-bit patterns and the host generator's state after each of 3 inputs, plan "generic";
  * two half-length runs equal one whole run (no norm in between: normalisation is not idempotent in a 16-bit format);
  * a Network.pipelined() section gives the same bits as synchronous runs;
  * the literal construct -> to("cuda") -> run sequence of batch_eth_mnist.py with w_dtype=torch.float16;
  * each kernel against the reference's torch statements on the CPU, over the sweeps of tests/test_half_hostcheck.py: N in {1, 7, 33, 40,
    400} (one column, odd row lengths, the 32-column class boundary, more than one 256-column workgroup), Nin in {17, 100, 784}, B in
    {1, 3, 33}, density in {0, 0.02, 0.3, 1}, accumulate on and off, the rule variants, a zero column, norm 78.4;
  * an inhibition sum beyond float16's range gives -inf, as torch does;
  * the device refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import half_cases as HC
from test_half_host import build, check_snapshots, gold, same
from test_half_hostcheck import DTYPES, same_bits, sweep_normalize, sweep_postpre, sweep_prop

pytestmark = pytest.mark.gpu
DEV = "cuda"


def to_dev(t):
    return t.to(DEV)


class DeviceImpl:
    """The three operations through bindsnet_amd.ops on device tensors."""

    def prop(self, W, s, out, accumulate):
        from bindsnet_amd import ops
        return ops.prop_cascade(W, s, out, accumulate=accumulate)

    def postpre(self, W, s_src, x_src, s_tgt, x_tgt, nu0, nu1, dt, decay, lo, hi):
        from bindsnet_amd import ops
        ops.stdp_postpre(W, s_src, x_src, s_tgt, x_tgt, nu0, nu1, use_dt=True, dt=dt, decay=decay, wmin=lo, wmax=hi)
        return W

    def normalize(self, W, norm):
        from bindsnet_amd import ops
        ops.normalize(W, norm, use_abs=False)
        return W


def monitor():
    from bindsnet_amd.network.monitors import Monitor
    return Monitor


@pytest.mark.parametrize("name", sorted(HC.CASES))
def test_fixture_cases_on_the_device(name):
    net = build(name)
    net.to(DEV)
    assert HC.value_of(net).is_cuda and HC.value_of(net).dtype == HC.dtype_of(name)
    snaps = HC.run_case(net, name, monitor(), device=DEV)
    assert net.last_plan == "generic"
    check_snapshots(name, snaps)


@pytest.mark.parametrize("name", ["a", "d"])
def test_two_half_runs_equal_one_whole_run(name):
    whole, halves = build(name, norm=None), build(name, norm=None)
    whole.to(DEV)
    halves.to(DEV)
    torch.manual_seed(3)
    a = HC.run_case(whole, name, monitor(), device=DEV, count=2)
    torch.manual_seed(3)
    b = HC.run_case(halves, name, monitor(), device=DEV, count=2, pieces=2)
    assert sum(int(s["sE"].sum()) for s in a) > 0 and not np.array_equal(a[0]["value"], a[1]["value"])
    for r, (x, y) in enumerate(zip(a, b)):
        for key in x:
            same(y[key], x[key], f"case {name} input {r}: {key}, two halves against the whole run")


def test_pipelined_section_gives_the_bits_of_synchronous_runs():
    name = "a"
    net = build(name)
    net.to(DEV)
    mon = monitor()(net.layers["Ae"], ["s"], time=HC.CASES[name]["T"])
    net.add_monitor(mon, "Ae_s")
    xs = [torch.from_numpy(HC.inputs(name, r)).to(DEV) for r in range(HC.N_IN)]
    rasters = []
    with net.pipelined():
        for x in xs:
            net.run({"X": x}, time=HC.CASES[name]["T"])
            rasters.append(mon.get("s"))
            net.reset_state_variables()
            assert net.last_plan == "generic"
    g = gold(name)
    for r, ras in enumerate(rasters):
        got = ras.cpu().numpy().reshape(-1).astype(np.uint8)
        same(got, np.unpackbits(g[f"r{r}_sE"])[:got.size], f"pipelined input {r}: Ae raster")
    same(HC.bits16(HC.value_of(net)), g[f"r{HC.N_IN - 1}_value"], "pipelined: the learned value")
    assert HC.sha(torch.get_rng_state().numpy()) == str(g[f"r{HC.N_IN - 1}_rng_sha"])


def test_the_example_s_construct_move_run_sequence():
    """examples/mnist/batch_eth_mnist.py --w_dtype float16: the constructor call, .to("cuda"), a batch through run()."""
    import warnings
    from bindsnet_amd.models import DiehlAndCook2015
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        network = DiehlAndCook2015(device="cpu", sparse=False, batch_size=4, n_inpt=784, n_neurons=100, exc=22.5, inh=120, dt=1.0, norm=78.4,
                                   nu=(1e-4, 1e-2), theta_plus=0.05, inpt_shape=(1, 28, 28), w_dtype=getattr(torch, "float16"))
    network.to("cuda")
    x = torch.from_numpy((np.random.default_rng(0).random((50, 4, 1, 28, 28)) < 0.12).astype(np.uint8)).to("cuda")
    before = HC.bits16(HC.value_of(network))
    network.run(inputs={"X": x}, time=50)
    assert network.last_plan == "generic"
    after = HC.value_of(network)
    assert after.dtype == torch.float16 and after.is_cuda and not np.array_equal(HC.bits16(after), before)
    sums = after.float().sum(0)
    assert torch.isfinite(sums).all() and float((sums - 78.4).abs().max()) < 1.0      # normalised, to float16's resolution


@pytest.mark.parametrize("N", HC.SWEEP_N)
@pytest.mark.parametrize("dtype", DTYPES)
def test_propagation_kernel_equals_torch(dtype, N):
    sweep_prop(DeviceImpl(), dtype, N, to=to_dev)


@pytest.mark.parametrize("B", HC.SWEEP_B)
@pytest.mark.parametrize("dtype", DTYPES)
def test_postpre_kernel_equals_torch(dtype, B):
    sweep_postpre(DeviceImpl(), dtype, B, to=to_dev)


@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_kernel_equals_torch(dtype):
    sweep_normalize(DeviceImpl(), dtype, to=to_dev)


def test_an_inhibition_sum_beyond_float16_gives_minus_infinity():
    W = torch.full((400, 7), -200.0, dtype=torch.float16)
    s = torch.ones(2, 400, dtype=torch.uint8)
    want = HC.ref_prop(W, s)
    assert torch.isinf(want).all() and (want < 0).all()
    got = DeviceImpl().prop(W.to(DEV), s.to(DEV), torch.zeros(2, 7, device=DEV), False).cpu()
    same_bits(got, want, "overflowing inhibition")


def test_device_refusals():
    from bindsnet_amd import _lib, ops
    from bindsnet_amd.network import Network
    from bindsnet_amd.network.monitors import Monitor
    from bindsnet_amd.network.nodes import Input, LIFNodes
    from bindsnet_amd.network.topology import MulticompartmentConnection
    from bindsnet_amd.network.topology_features import Mask, Weight
    L = _lib.lib()
    one = torch.zeros(8, device=DEV)
    p = C.c_void_p(one.data_ptr())
    assert L.snn_prop_cascade_h16(p, 0, p, p, 1, 1, 1, 0, None) == -1          # w_dtype 0 is not a half
    assert L.snn_prop_cascade_h16(p, 3, p, p, 1, 1, 1, 0, None) == -1
    assert L.snn_stdp_postpre_h16(p, 1, p, p, p, p, 300, 4, 4, 0.1, 0.1, 1, 1.0, 1.0, 0, 0.0, 0, 0.0, None) == -2     # B > 256
    assert L.snn_normalize_h16(p, 1, 1, 1, 1.0, None, None) == -1
    with pytest.raises(NotImplementedError, match="float16"):
        ops.normalize(torch.ones(4, 4, dtype=torch.float16, device=DEV), 1.0, use_abs=True)
    with pytest.raises(TypeError):
        ops.prop_cascade(torch.ones(4, 4, dtype=torch.float64, device=DEV), torch.ones(1, 4, dtype=torch.uint8, device=DEV), torch.zeros(1, 4, device=DEV))

    def net_of(pipeline):
        X, Y = Input(n=6, traces=True), LIFNodes(n=5, traces=True)
        net = Network()
        net.add_layer(X, "X")
        net.add_layer(Y, "Y")
        net.add_connection(MulticompartmentConnection(X, Y, device="cpu", pipeline=pipeline), "X", "Y")
        return net.to(DEV), Y

    x = torch.ones(3, 2, 6, dtype=torch.uint8, device=DEV)
    for dtype in DTYPES:
        w = torch.rand(6, 5).to(dtype)
        # a multi-feature pipeline with a half value: today's message, which names the dtype
        net, Y = net_of([Weight("w", w.clone(), value_dtype=dtype), Mask("m", torch.ones(6, 5, dtype=torch.bool)), Weight("g", torch.rand(6, 5))])
        with pytest.raises(NotImplementedError, match=str(dtype)):
            net.run({"X": x.clone()}, time=3)
        assert bool((Y.v == Y.rest).all())                  # no step ran (the state was only sized for the batch)
        # a Monitor on the half value
        feat = Weight("w", w.clone(), value_dtype=dtype)
        net, Y = net_of([feat])
        net.add_monitor(Monitor(feat, ["value"], time=3), "value")
        with pytest.raises(NotImplementedError, match=str(dtype)):
            net.run({"X": x.clone()}, time=3)
        del net.monitors["value"]
        net.run({"X": x.clone()}, time=3)                   # ... without it the network runs
        assert net.last_plan == "generic"
    # float64 stays refused
    net, Y = net_of([Weight("w", torch.rand(6, 5).double(), value_dtype=torch.float64)])
    with pytest.raises(NotImplementedError, match="float64"):
        net.run({"X": x.clone()}, time=3)
