"""Network._preflight on the HOST: every reason the package gives against a run before it starts, asked through the one hook
(`_refusals(key, request)` of every connection, rule and layer, then the network's own questions), with no GPU.

* One row per refusal: the smallest network that triggers it, a request with on_device=True (the device-only refusals touch no
  device), the exception type and the wording the existing device and host tests look for; every tensor of every layer and
  connection and the batch size are what they were.
* Through Network.run on the host, the refusals that depend on the batch size: batch_size, the state's shapes and a monitor's
  recording are those of before the call.
* The class-level facts that replaced type ladders: the tensors the descriptor cache watches per node class (the table below was
  taken from the sixteen-name union the cache used to probe on every layer), and the classes whose reset is one fill launch.
* A host network that runs gives no reason at all."""
import inspect
import re

import pytest
import torch

from bindsnet_amd import conversion, learning
from bindsnet_amd.learning import MCC_learning
from bindsnet_amd.network import Network, nodes, topology, topology_features
from bindsnet_amd.network._preflight import RunRequest
from bindsnet_amd.network.monitors import Monitor

T = 3


def _net(X, Y, conn_of, B=2, name_y="Y", **kw):
    net = Network(dt=kw.pop("dt", 1.0), batch_size=B, **kw)
    net.add_layer(X, "X")
    net.add_layer(Y, name_y)
    conn = conn_of(X, Y)
    if conn is not None:
        net.add_connection(conn, "X", name_y)
    return net


def _spikes(*shape, B=2):
    return {"X": torch.ones(T, B, *shape, dtype=torch.uint8)}


def _real(*shape, B=2):
    return {"X": torch.rand(T, B, *shape)}


def _tensors(net):
    """Every tensor held by a layer, a connection, a feature or a rule of the network, by a name that says where."""
    out = {}
    owners = [(f"layer {k}", l) for k, l in net.layers.items()] + [(f"conn {k}", c) for k, c in net.connections.items()]
    for k, c in net.connections.items():
        owners += [(f"feature {k} {f.name}", f) for f in getattr(c, "pipeline", ())]
        owners.append((f"rule {k}", c._rule()))
    for where, obj in owners:
        held = dict(vars(obj))
        held.update(getattr(obj, "_buffers", {}))
        held.update(getattr(obj, "_parameters", {}))
        for name, t in held.items():
            if isinstance(t, torch.Tensor):
                out[f"{where}.{name}"] = t
    return out


def _snapshot(net):
    return {k: (t.to_dense() if t.is_sparse else t).detach().clone() for k, t in _tensors(net).items()}, net.batch_size


def _unchanged(net, before):
    tensors, B = before
    now = _tensors(net)
    assert net.batch_size == B and now.keys() == tensors.keys()
    for k, t in now.items():
        t = t.to_dense() if t.is_sparse else t
        assert t.shape == tensors[k].shape and t.dtype == tensors[k].dtype and torch.equal(t, tensors[k]), k


# ---- the rows: name -> () -> (network, inputs, {masks, injects_v}, exception type, wording) ------------------------------------

def _sparse(**kw):
    w = (torch.rand(12, 6) * (torch.rand(12, 6) < 0.5)).to_sparse()
    return _net(nodes.Input(n=12, traces=True), nodes.LIFNodes(n=6, traces=True), lambda a, b: topology.SparseConnection(a, b, w=w, **kw))


def _monitored(net, var="w"):
    net.add_monitor(Monitor(net.connections[("X", "Y")], [var], time=T), "m")
    return net


def _sparse_double():
    net = _sparse()
    conn = net.connections[("X", "Y")]
    conn.w = torch.nn.Parameter(conn.w.double(), requires_grad=False)
    return net


def _pool(shape=(2, 4, 4), B=2, target=None, **kw):
    X = nodes.Input(shape=shape, traces=True)
    Y = nodes.LIFNodes(shape=target or (shape[0], shape[1] // 2 or 1, shape[2] // 2), traces=True)
    kw.setdefault("decay", 0.2)
    return _net(X, Y, lambda a, b: topology.MaxPool2dConnection(a, b, kernel_size=2, stride=2, **kw), B=B)


def _mean(**kw):
    return _net(nodes.Input(n=6, traces=True), nodes.LIFNodes(n=3, traces=True), lambda a, b: topology.MeanFieldConnection(a, b, **kw))


def _permute(extra=None, conn_of=None):
    X, P = nodes.Input(shape=(2, 3, 5)), conversion.PassThroughNodes(shape=(5, 2, 3))
    net = _net(X, P, conn_of or (lambda a, b: conversion.PermuteConnection(a, b, dims=(0, 3, 1, 2))), name_y="P")
    if extra is not None:
        net.add_layer(nodes.Input(shape=(2, 3, 5)), "X2")
        net.add_connection(conversion.PermuteConnection(net.layers["X2"], P, dims=(0, 3, 1, 2)), "X2", "P")
    return net


def _half(dtype=torch.float16, monitor=False, **later):
    """A float16 / bfloat16 Weight; `later`: attributes set behind the constructor, which refuses them itself."""
    X, Y = nodes.Input(n=6, traces=True), nodes.LIFNodes(n=5, traces=True)
    feat = topology_features.Weight("w", torch.rand(6, 5).to(dtype), value_dtype=dtype)
    for key, value in later.items():
        setattr(feat, key, value)
    net = _net(X, Y, lambda a, b: topology.MulticompartmentConnection(a, b, device="cpu", pipeline=[feat]))
    if monitor == "value":
        net.add_monitor(Monitor(feat, ["value"], time=T), "m")
    elif monitor:
        net.add_monitor(Monitor(net.connections[("X", "Y")], ["w"], time=T), "m")
    return net


def _mcc():
    feat = topology_features.Weight("w", value=torch.rand(12, 6))
    return _net(nodes.Input(n=12, traces=True), nodes.LIFNodes(n=6, traces=True),
                lambda a, b: topology.MulticompartmentConnection(a, b, device="cpu", pipeline=[feat]))


def _dense(target=None, n_in=12, B=2, **kw):
    Y = target or nodes.LIFNodes(n=6, traces=True)
    return _net(nodes.Input(n=n_in, traces=True), Y, lambda a, b: topology.Connection(a, b, w=torch.rand(n_in, Y.n), **kw), B=B)


def _conv3d():
    X, Y = nodes.Input(shape=(1, 3, 3, 3), traces=True), nodes.LIFNodes(shape=(2, 2, 2, 2), traces=True)
    return _net(X, Y, lambda a, b: topology.Conv3dConnection(a, b, kernel_size=2, update_rule=learning.PostPre, nu=(1e-2, 1e-2)), B=1)


def _csrm_window_of_another_batch():
    net = _dense(target=nodes.CSRMNodes(n=6, traces=True))
    net.connections[("X", "Y")].s_w = torch.zeros(3, 20, 12)
    return net


def _csrm_sparse():
    w = torch.rand(12, 6).to_sparse()
    return _net(nodes.Input(n=12, traces=True), nodes.CSRMNodes(n=6, traces=True), lambda a, b: topology.SparseConnection(a, b, w=w))


def _pool_other_rates():
    net = _pool()
    net.connections[("X", "Y")].firing_rates = torch.zeros(3, 2, 4, 4)      # (at the network's own batch size: nothing else is out of step)
    return net


def _rmax(B=1):
    X, Y = nodes.Input(n=6, traces=True, traces_additive=True), nodes.SRM0Nodes(n=4, traces=True)
    return _net(X, Y, lambda a, b: topology.Connection(a, b, w=torch.rand(6, 4), update_rule=learning.Rmax, nu=1e-2), B=B)


def _postpre_source_rates(B=2):
    net = _dense(update_rule=learning.PostPre, nu=(1e-2, 1e-2), reduction=torch.sum, B=B)
    net.connections[("X", "Y")].update_rule.nu = torch.full((2, 12, 1), 1e-2)
    return net


def _wdpostpre_infinite_bound():
    net = _dense(update_rule=learning.WeightDependentPostPre, nu=(1e-2, 1e-2), reduction=torch.sum, wmin=torch.zeros(12, 6), wmax=torch.ones(12, 6))
    net.connections[("X", "Y")].wmax[0, 0] = float("inf")
    return net


def _sparse_w(w):
    net = _sparse()
    net.connections[("X", "Y")].w = torch.nn.Parameter(w, requires_grad=False)
    return net


def _half_mstdp(rule):
    """A reward-modulated MCC rule whose float32 Weight was cast to float16 behind the constructor, which refuses it itself."""
    X, Y = nodes.Input(n=6, traces=True), nodes.LIFNodes(n=5, traces=True)
    feat = topology_features.Weight("w", torch.rand(6, 5), learning_rule=rule, nu=(1e-2, 1e-2), range=[0.0, 1.0])
    net = _net(X, Y, lambda a, b: topology.MulticompartmentConnection(a, b, device="cpu", pipeline=[feat]), B=1)
    feat.value = feat.value.half()
    return net


def _conv3d_unfold_mismatch():
    """A kernel that is no cube: the reference unfolds depth with the kernel's width, so its bmm operands have 6 rows against 8 positions."""
    X, Y = nodes.Input(shape=(1, 4, 3, 3), traces=True), nodes.LIFNodes(shape=(2, 2, 2, 2), traces=True)
    return _net(X, Y, lambda a, b: topology.Conv3dConnection(a, b, kernel_size=(3, 2, 2), update_rule=learning.PostPre, nu=(0.0, 1e-2)), B=1)


def _csrm_last_spikes():
    net = _dense(target=nodes.CSRMNodes(n=6, traces=True))
    net.layers["Y"].last_spikes = torch.zeros(2, 3, 6)
    return net


def _csrm_window(shape):
    net = _dense(target=nodes.CSRMNodes(n=6, traces=True))
    net.connections[("X", "Y")].s_w = torch.zeros(*shape)
    return net


def _mean_large():
    """4096 source neurons at batch 4097, one element past 2^24; the input is one byte, expanded."""
    net = _net(nodes.Input(n=4096), nodes.LIFNodes(n=3), lambda a, b: topology.MeanFieldConnection(a, b, w=torch.tensor(0.5)))
    return net, {"X": torch.zeros(1, 1, 1, dtype=torch.uint8).expand(T, 4097, 4096)}


def _permute_monitored():
    net = _permute()
    net.add_monitor(Monitor(net.connections[("X", "P")], ["dims"], time=T), "m")
    return net


def _csrm_tensor_rest():
    net = _dense(target=nodes.CSRMNodes(n=6, traces=True))
    net.layers["Y"].rest = torch.full((6,), -65.0)
    return net


ROWS = {
    # what a family cannot run at all (its mask, a monitor on it, its own settings)
    "sparse_norm": lambda: (_sparse(norm=2.0), _spikes(12), {}, NotImplementedError, r"normalize\(\) raises"),
    "sparse_mask": lambda: (_sparse(), _spikes(12), {"masks": {("X", "Y"): torch.ones(12, 6)}}, Exception, "Mask isn't supported"),
    "sparse_monitor": lambda: (_monitored(_sparse()), _spikes(12), {}, NotImplementedError, "monitor"),
    "sparse_float64": lambda: (_sparse_double(), _spikes(12), {}, NotImplementedError, "float32"),
    "pool_mask": lambda: (_pool(), _spikes(2, 4, 4), {"masks": {("X", "Y"): torch.zeros(1, dtype=torch.bool)}}, NotImplementedError, "mask"),
    "pool_monitor": lambda: (_monitored(_pool(), "firing_rates"), _spikes(2, 4, 4), {}, NotImplementedError, "monitor"),
    "mean_norm": lambda: (_mean(w=torch.tensor(0.5), norm=1.0), _spikes(6), {}, NotImplementedError, "TypeError"),
    "mean_mask": lambda: (_mean(w=torch.tensor(0.5)), _spikes(6), {"masks": {("X", "Y"): torch.zeros(1, dtype=torch.bool)}}, NotImplementedError, "mask"),
    "mean_monitor": lambda: (_monitored(_mean(w=torch.tensor(0.5))), _spikes(6), {}, NotImplementedError, "monitor"),
    "gather_mask": lambda: (_permute(), _spikes(2, 3, 5), {"masks": {("X", "P"): torch.ones(30, 30)}}, NotImplementedError, "mask"),
    "gather_monitor": lambda: (_permute_monitored(), _spikes(2, 3, 5), {}, NotImplementedError, "monitor"),
    "gather_geometry": lambda: (_permute(conn_of=lambda a, b: conversion.PermuteConnection(a, b, dims=(1, 0, 2, 3))), _spikes(2, 3, 5), {}, NotImplementedError, "dims"),
    "gather_shape": lambda: (_permute(conn_of=lambda a, b: conversion.PermuteConnection(a, b, dims=(0, 2, 3, 1))), _spikes(2, 3, 5), {}, RuntimeError, "shape"),
    "sparse_w_shape": lambda: (_sparse_w(torch.rand(6, 12).to_sparse()), _spikes(12), {}, NotImplementedError, "sparse COO tensor of shape"),
    "sparse_w_dense": lambda: (_sparse_w(torch.rand(12, 6)), _spikes(12), {}, NotImplementedError, "sparse COO tensor of shape"),
    "half_mstdp": lambda: (_half_mstdp(MCC_learning.MSTDP), _spikes(6, B=1), {}, NotImplementedError, "MCC MSTDP on a torch.float16"),
    "half_mstdpet": lambda: (_half_mstdp(MCC_learning.MSTDPET), _spikes(6, B=1), {}, NotImplementedError, "MCC MSTDPET on a torch.float16"),
    "half_monitor": lambda: (_half(monitor=True), _spikes(6), {}, NotImplementedError, "float16"),
    "half_tensor_norm": lambda: (_half(norm=torch.ones(5)), _spikes(6), {}, NotImplementedError, "float16"),
    "half_norm_step": lambda: (_half(torch.bfloat16, norm=1.0, norm_frequency="time step"), _spikes(6), {}, NotImplementedError, "bfloat16"),
    # ... cannot learn
    "conv3d_postpre": lambda: (_conv3d(), _spikes(1, 3, 3, 3, B=1), {}, RuntimeError, "float != bool"),
    "conv3d_unfold": lambda: (_conv3d_unfold_mismatch(), _spikes(1, 4, 3, 3, B=1), {}, RuntimeError, "fails in the reference"),
    # ... into a layer that gathers a window
    "csrm_no_window": lambda: (_csrm_sparse(), _spikes(12), {}, NotImplementedError, "compute_window"),
    "csrm_window_batch": lambda: (_csrm_window_of_another_batch(), _spikes(12), {}, RuntimeError, "Sizes of tensors must match"),
    "csrm_window_length": lambda: (_csrm_window((2, 7, 12)), _spikes(12), {}, RuntimeError, "Sizes of tensors must match"),
    # ... out of a real-valued Input (device only)
    "analog_sparse": lambda: (_sparse(), _real(12), {}, NotImplementedError, "SparseConnection.*uint8 or bool"),
    "analog_mcc": lambda: (_mcc(), _real(12), {}, NotImplementedError, "MulticompartmentConnection.*uint8 or bool"),
    "analog_permute": lambda: (_permute(), _real(2, 3, 5), {}, NotImplementedError, "PermuteConnection.*uint8 or bool"),
    "analog_rule": lambda: (_dense(update_rule=learning.PostPre, nu=(1e-2, 1e-2), reduction=torch.sum), _real(12), {}, NotImplementedError, "PostPre"),
    "analog_csrm": lambda: (_dense(target=nodes.CSRMNodes(n=6)), _real(12), {}, NotImplementedError, "CSRMNodes"),
    # ... at this batch size
    "pool_decay": lambda: (_pool(decay=None), _spikes(2, 4, 4), {}, TypeError, "decay"),
    "pool_squeeze": lambda: (_pool((1, 4, 4)), _spikes(1, 4, 4), {}, RuntimeError, "squeeze"),
    "pool_target": lambda: (_pool(target=(8,)), _spikes(2, 4, 4), {}, RuntimeError, "target's shape"),
    "pool_rates": lambda: (_pool_other_rates(), _spikes(2, 4, 4), {}, RuntimeError, "firing_rates has shape"),
    "pool_source_rank": lambda: (_net(nodes.Input(shape=(4, 4)), nodes.LIFNodes(shape=(2, 2)), lambda a, b: topology.MaxPool2dConnection(a, b, kernel_size=2, stride=2, decay=0.2)),
                                 _spikes(4, 4), {}, RuntimeError, "source's shape must be"),
    "mean_2_24": lambda: (*_mean_large(), {}, NotImplementedError, "2\\^24"),
    "mean_w_shape": lambda: (_mean(w=torch.rand(5)), _spikes(6), {}, NotImplementedError, "tail"),
    # the rules
    "rmax_batch": lambda: (_rmax(), {"X": torch.ones(T, 2, 6, dtype=torch.uint8)}, {}, NotImplementedError, r"view\(-1\)"),
    "postpre_source_rates": lambda: (_postpre_source_rates(), _spikes(12), {}, RuntimeError, "does not broadcast"),
    "wdpostpre_bound": lambda: (_wdpostpre_infinite_bound(), _spikes(12), {}, NotImplementedError, "finite wmin and wmax for every synapse"),
    # the layers
    "csrm_kernels": lambda: (_net(nodes.Input(n=12, traces=True), nodes.CSRMNodes(n=6), lambda a, b: topology.Connection(a, b, w=torch.rand(12, 6)), dt=0.5),
                             {"X": torch.ones(2 * T, 2, 12, dtype=torch.uint8)}, {}, RuntimeError, r"einsum\(\)"),
    "csrm_last_spikes": lambda: (_csrm_last_spikes(), _spikes(12), {}, RuntimeError, "last_spikes has shape"),
    "csrm_current": lambda: (_dense(target=nodes.CSRMNodes(n=6)), dict(_spikes(12), Y=torch.zeros(T, 2, 6)), {}, NotImplementedError, r"inputs\['Y'\]"),
    "csrm_tensor_rest": lambda: (_csrm_tensor_rest(), _spikes(12), {}, NotImplementedError, "rest"),
    "pass_current": lambda: (_permute(), dict(_spikes(2, 3, 5), P=torch.zeros(T, 2, 30)), {}, NotImplementedError, "external current"),
    "pass_injects_v": lambda: (_permute(), _spikes(2, 3, 5), {"injects_v": {"P": torch.ones(30)}}, NotImplementedError, "injects_v"),
    "pass_two_feeders": lambda: (_permute(extra=True), dict(_spikes(2, 3, 5), X2=torch.ones(T, 2, 2, 3, 5, dtype=torch.uint8)), {}, NotImplementedError, "exactly one"),
    "pass_dense_feeder": lambda: (_permute(conn_of=lambda a, b: topology.Connection(a, b, w=torch.rand(30, 30))), _spikes(2, 3, 5), {}, NotImplementedError,
                                  "Connection into PassThroughNodes"),
    # what only the network can tell
    "half_value_monitor": lambda: (_half(monitor="value"), _spikes(6), {}, NotImplementedError, "float16"),
    "analog_no_reader": lambda: (_net(nodes.Input(n=12), nodes.LIFNodes(n=6), lambda a, b: None), _real(12), {}, NotImplementedError, "no Connection or Conv2dConnection reads"),
    "analog_float64": lambda: (_dense(), {"X": torch.rand(T, 2, 12).double()}, {}, NotImplementedError, r"\.float\(\)"),
}


@pytest.mark.parametrize("name", ROWS)
def test_refusal_is_given_before_anything_changes(name):
    net, inputs, kw, exc, wording = ROWS[name]()
    before = _snapshot(net)
    rng = torch.get_rng_state()
    req = RunRequest.of(net, inputs, T, kw.get("masks"), kw.get("injects_v"), on_device=True)
    try:
        err = next(iter(net._preflight(req)), None)
    except Exception as raised:                            # (a question that raises its answer itself)
        err = raised
    assert type(err) is exc or (exc is not Exception and isinstance(err, exc)), f"{name}: {err!r}"
    assert re.search(wording, str(err)), f"{name}: {err}"
    _unchanged(net, before)
    assert torch.equal(torch.get_rng_state(), rng)


def test_device_only_refusals_are_not_asked_of_a_host_run():
    for name in ("analog_sparse", "analog_rule", "csrm_current", "pass_two_feeders", "analog_float64"):
        net, inputs, kw, _, _ = ROWS[name]()
        req = RunRequest.of(net, inputs, T, kw.get("masks"), kw.get("injects_v"))
        assert not req.on_device and list(net._preflight(req)) == [], name


# ---- refusals that depend on the batch size, through Network.run on the host --------------------------------------------------

def _pool_1_to_3():
    """Input (1, 4, 4) -> MaxPool2dConnection(2, stride 2) -> LIFNodes (1, 2, 2) at batch size 1; one good run fills the monitor,
    then the connection loses its `decay` and is run at batch size 3."""
    net = _pool((1, 4, 4), B=1, decay=0.5)
    return net, {"X": torch.ones(T, 1, 1, 4, 4, dtype=torch.uint8)}, lambda: setattr(net.connections[("X", "Y")], "decay", None), \
        {"X": torch.ones(T, 3, 1, 4, 4, dtype=torch.uint8)}, TypeError, "needs `decay=`"


def _rmax_1_to_2():
    net = _rmax()
    return net, {"X": torch.ones(T, 1, 6, dtype=torch.uint8)}, lambda: None, {"X": torch.ones(T, 2, 6, dtype=torch.uint8)}, \
        NotImplementedError, r"view\(-1\)"


def _postpre_1_to_3():
    net = _dense(update_rule=learning.PostPre, nu=(1e-2, 1e-2), reduction=torch.sum, B=1)
    return net, {"X": torch.ones(T, 1, 12, dtype=torch.uint8)}, \
        lambda: setattr(net.connections[("X", "Y")].update_rule, "nu", torch.full((2, 12, 1), 1e-2)), \
        {"X": torch.ones(T, 3, 12, dtype=torch.uint8)}, RuntimeError, "does not broadcast"


@pytest.mark.parametrize("make", (_pool_1_to_3, _rmax_1_to_2, _postpre_1_to_3), ids=lambda f: f.__name__.strip("_"))
def test_a_batch_size_refusal_leaves_batch_size_state_and_recordings(make):
    net, good, spoil, refused, exc, wording = make()
    mon = Monitor(net.layers["Y"], ["s", "v"], time=T)
    net.add_monitor(mon, "Y")
    net.run(good, time=T, reward=1.0)
    spoil()
    before, recorded = _snapshot(net), {v: mon.get(v).clone() for v in ("s", "v")}
    assert recorded["v"].shape[:2] == (T, 1) and net.batch_size == 1
    with pytest.raises(exc, match=wording):
        net.run(refused, time=T, reward=1.0)
    _unchanged(net, before)
    assert net.layers["Y"].v.shape[0] == 1 and net.layers["X"].s.shape[0] == 1
    for v in ("s", "v"):
        assert not mon.clean and torch.equal(mon.get(v), recorded[v]), v


def test_reward_function_is_not_asked_for_a_refused_run():
    class Reward:
        calls = 0

        def compute(self, **kwargs):
            Reward.calls += 1
            return 1.0

        def update(self, **kwargs):
            pass
    net = _rmax()
    net.reward_fn = Reward()
    with pytest.raises(NotImplementedError, match=r"view\(-1\)"):
        net.run({"X": torch.ones(T, 2, 6, dtype=torch.uint8)}, time=T)
    assert Reward.calls == 0 and net.batch_size == 1


# ---- what replaced the type ladders ---------------------------------------------------------------------------------------------

# Per node class: which of "v", "refrac_count", "x", "theta", "i", "u", "a", "b", "c", "d", "s_prob", "rho", "last_spikes", "resKernel",
# "refKernel", "summed" -- the union the descriptor cache probed on every layer -- are tensors of a layer with traces (and, where the
# class takes it, sum_input) once its descriptor is built.
WATCHED = {
    "Input": {"x"},
    "McCullochPitts": {"v", "x"},
    "IFNodes": {"v", "refrac_count", "x"},
    "LIFNodes": {"v", "refrac_count", "x"},
    "BoostedLIFNodes": {"v", "refrac_count", "x"},
    "CurrentLIFNodes": {"v", "refrac_count", "i", "x"},
    "AdaptiveLIFNodes": {"v", "refrac_count", "theta", "x"},
    "DiehlAndCookNodes": {"v", "refrac_count", "theta", "x"},
    "IzhikevichNodes": {"v", "u", "a", "b", "c", "d", "x"},
    "SRM0Nodes": {"v", "refrac_count", "s_prob", "rho", "x"},
    "CSRMNodes": {"v", "theta", "last_spikes", "resKernel", "refKernel", "x"},
    "SubtractiveResetIFNodes": {"v", "refrac_count", "summed", "x"},
    "PassThroughNodes": {"v", "x"},
}


def _node_classes():
    from bindsnet_amd.conversion import nodes as conversion_nodes
    return {name: cls for mod in (nodes, conversion_nodes) for name, cls in inspect.getmembers(mod, inspect.isclass)
            if issubclass(cls, nodes.Nodes) and cls is not nodes.Nodes and cls.__module__ == mod.__name__ and not name.startswith("_")}


def _layer(cls, B=2):
    layer = cls(n=4, traces=True, **({"sum_input": True} if cls._SUMS_INPUT else {}))
    layer.compute_decays(1.0)
    layer.set_batch_size(B)
    if hasattr(layer, "_prob_buffers"):
        layer._prob_buffers()                             # (SRM0Nodes: made when the descriptor is built)
    return layer


def test_every_node_class_names_the_tensors_the_descriptor_cache_watches():
    classes = _node_classes()
    assert set(classes) == set(WATCHED)
    for name, cls in classes.items():
        assert set(_layer(cls)._watched()) == WATCHED[name], name
    bare = nodes.LIFNodes(n=4)                            # (without traces there is no `x` to watch)
    bare.set_batch_size(2)
    assert set(bare._watched()) == {"v", "refrac_count"}


def test_the_one_launch_reset_covers_the_four_stock_classes_only():
    classes = _node_classes()
    filled = {name for name, cls in classes.items() if _layer(cls)._reset_fill() is not None}
    assert filled == {"Input", "LIFNodes", "DiehlAndCookNodes", "AdaptiveLIFNodes"}

    class MyLIF(nodes.LIFNodes):                          # (a subclass may keep state of its own: its reset is called)
        pass
    assert _layer(MyLIF)._reset_fill() is None
    lif = _layer(nodes.LIFNodes)
    lif.rest.fill_(-60.0)
    import struct
    assert [(t.data_ptr(), pat) for t, pat in lif._reset_fill()] == \
        [(lif.s.data_ptr(), 0), (lif.x.data_ptr(), 0), (lif.refrac_count.data_ptr(), 0), (lif.v.data_ptr(), struct.unpack("<I", struct.pack("<f", -60.0))[0])]
    inp = _layer(nodes.Input)
    assert [(t.data_ptr(), pat) for t, pat in inp._reset_fill()] == [(inp.s.data_ptr(), 0), (inp.x.data_ptr(), 0)]


def test_facts_default_to_nothing_and_are_set_where_the_issue_says():
    conns = [c for _, c in inspect.getmembers(topology, inspect.isclass) if issubclass(c, (topology.AbstractConnection, topology.AbstractMulticompartmentConnection))]
    conns += [conversion.PermuteConnection, conversion.ConstantPad2dConnection]
    assert {c.__name__ for c in conns if c._takes_real} == {"Connection", "Conv2dConnection"}
    assert {c.__name__ for c in conns if c._has_window} == {"Connection"}
    assert {n for n, c in _node_classes().items() if c._gathers_window} == {"CSRMNodes"}
    rules = [c for mod in (learning.learning, MCC_learning) for _, c in inspect.getmembers(mod, inspect.isclass)
             if issubclass(c, (learning.LearningRule, MCC_learning.MCC_LearningRule))]
    assert {c.__name__ for c in rules if not c._learns} == {"NoOp"} and len([c for c in rules if not c._learns]) == 2


# ---- a network that runs gives no reason ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("make,inputs", [(lambda: _dense(update_rule=learning.PostPre, nu=(1e-2, 1e-2), reduction=torch.sum), _spikes(12)),
                                         (lambda: _pool(), _spikes(2, 4, 4)), (lambda: _dense(target=nodes.CSRMNodes(n=6, traces=True)), _spikes(12)),
                                         (_permute, _spikes(2, 3, 5)), (lambda: _rmax(), {"X": torch.ones(T, 1, 6, dtype=torch.uint8)})],
                         ids=["postpre", "pool", "csrm", "permute", "rmax"])
def test_a_passing_host_network_yields_nothing(make, inputs):
    net = make()
    req = RunRequest.of(net, inputs, T)
    assert (req.T, req.B, req.on_device, req.learning) == (T, inputs["X"].shape[1], False, True)
    assert list(net._preflight(req)) == []
    net.run(inputs, time=T, reward=1.0)
    assert net.last_plan == "host-torch"
