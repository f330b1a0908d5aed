"""`Network`: API mirror of bindsnet/network/network.py.

`run()` does not loop over timesteps in Python.  It translates the network (layers and
connections in insertion order, monitors, keyword arguments) into the descriptor arrays of
include/snnhip.h and makes ONE call to snn_net_run, which executes all T timesteps on the
device (bindsnet/network/network.py:380-465 restated in bindsnet_amd/csrc/snn_run.hip).
Anything the kernels do not implement raises NotImplementedError -- there is no fallback.
"""
import ctypes as C
import os
import tempfile
from typing import Dict, Optional, Type

import torch

from .. import _lib
from .._lib import dptr as _dptr
from ..rng import DeviceGenerator
from . import host_path
from ._preflight import RunRequest, is_analog
from .monitors import AbstractMonitor, Monitor, NetworkMonitor
from .nodes import Input, Nodes


def load(file_name: str, map_location: str = "cpu", learning: bool = None) -> "Network":
    """Reference: network.py:12-28 (whole-object pickle)."""
    network = torch.load(open(file_name, "rb"), map_location=map_location, weights_only=False)
    if learning is not None and "learning" in vars(network):
        network.learning = learning
    return network


_DESC_CACHE = os.environ.get("SNN_DESC_CACHE", "1") != "0"      # developer switch: rebuild the descriptors on every call


class _Pipeline:
    """State of a Network.pipelined() section: the runs enqueued since the last settlement."""

    def __init__(self, depth: int):
        self.depth = max(1, int(depth))
        self.pending = []              # plan name of every unsettled run, in order
        self.status = None             # device int32 [2 * depth]: {first attempt, second attempt} status words per run
        self.block = self.host = None  # the generator block on the device / its page-locked host image
        self.host0 = None              # host generator state at the start of the batch (None: no run of the batch draws)
        self.enabled = False
        self.stream = None             # the stream the batch's runs were enqueued on (settlement waits for THAT stream)


class Network(_lib.TouchingModule, torch.nn.Module):
    def __init__(self, dt: float = 1.0, batch_size: int = 1, learning: bool = True,
                 reward_fn: Optional[Type] = None) -> None:
        super().__init__()
        self.dt, self.batch_size = dt, batch_size
        self.layers, self.connections, self.monitors = {}, {}, {}
        self.train(learning)
        self.reward_fn = reward_fn() if reward_fn is not None else None
        self.last_plan = None          # name of the device plan the last run() used

    # ------------------------------------------------------------------ construction (network.py:119-161)
    def add_layer(self, layer: Nodes, name: str) -> None:
        self.layers[name] = layer
        self.add_module(name, layer)
        layer.train(self.learning)
        layer.compute_decays(self.dt)
        layer.set_batch_size(self.batch_size)

    def add_connection(self, connection, source: str, target: str) -> None:
        self.connections[(source, target)] = connection
        self.add_module(source + "_to_" + target, connection)
        connection.dt = self.dt
        connection.train(self.learning)

    def add_monitor(self, monitor: AbstractMonitor, name: str) -> None:
        self.monitors[name] = monitor
        monitor.network = self
        monitor.dt = self.dt

    def save(self, file_name: str) -> None:
        torch.save(self, open(file_name, "wb"))

    def clone(self) -> "Network":
        f = tempfile.SpooledTemporaryFile()
        torch.save(self, f)
        f.seek(0)
        return torch.load(f, weights_only=False)

    def prop_stats(self) -> dict:
        """Connection.prop_stats() of every connection that keeps them, by connection key: which body -- matrix cores or
        event-driven -- the generic plan's dense propagation took, in (tile of 16 samples, timestep) pairs."""
        return {key: c.prop_stats() for key, c in self.connections.items() if hasattr(c, "prop_stats")}

    def reset_prop_stats(self) -> None:
        for c in self.connections.values():
            if hasattr(c, "reset_prop_stats"):
                c.reset_prop_stats()

    _TRANSIENT = ("_workspace", "_scratch_pool", "_keep", "last_plan", "resident_retries", "lean_retries", "_lean_cooldown",
                  "_run_cache", "_reset_cache", "_shard_state", "_defer_norm", "_pipe", "_ws_state")

    def __getstate__(self):
        """save() / clone() pickle the whole object like the reference (network.py:163-209); device scratch, the
        workspace of the fused plans and the references that keep the last inputs alive are not model state."""
        state = dict(self.__dict__)
        for k in self._TRANSIENT:
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.last_plan = None

    def reset_state_variables(self) -> None:
        """Reference: network.py:467-481.  The state tensors of the layers that name them (Nodes._reset_fill: the stock classes'
        s, x, refrac_count <- 0, v <- rest; theta is NOT reset, nodes.py:1113-1120) are filled by ONE launch (snn_fill_segments)
        instead of four small fills per layer.  The segment table is kept while nothing has been assigned to a network object
        (_lib.epoch()); only Input.s, which aliases the last input slice of the previous run, is looked up again."""
        plan = self.__dict__.get("_reset_cache")
        if plan is None or plan["epoch"] != _lib.epoch() or not _DESC_CACHE:
            segs, others, rebind = [], [], []
            for l in self.layers.values():
                fill = l._reset_fill() if l.s.is_cuda and l.s.is_contiguous() else None
                if fill is None:
                    others.append(l)
                else:
                    if isinstance(l, Input):
                        rebind.append((len(segs), l))
                    segs += fill
            arr = None
            if segs and all(t.is_contiguous() for t, _ in segs) and len(segs) <= _lib.MAX_FILL_SEGMENTS:
                arr = (_lib.FillSegment * len(segs))()
                for k, (t, pat) in enumerate(segs):
                    arr[k].ptr, arr[k].bytes, arr[k].pattern = t.data_ptr(), t.numel() * t.element_size(), pat
            plan = {"epoch": _lib.epoch(), "segs": segs, "arr": arr, "others": others, "rebind": rebind,
                    "rests": [(l.rest, l.rest._version) for l in self.layers.values()
                              if isinstance(getattr(l, "rest", None), torch.Tensor)]}
            self.__dict__["_reset_cache"] = plan if all(t._version == v for t, v in plan["rests"]) else None
        elif any(t._version != v for t, v in plan["rests"]):     # layer.rest changed in place: rebuild next time, and now
            self.__dict__["_reset_cache"] = None
            return self.reset_state_variables()
        else:
            for k, l in plan["rebind"]:
                s = l.s
                if not (s.is_cuda and s.is_contiguous()):
                    self.__dict__["_reset_cache"] = None
                    return self.reset_state_variables()
                plan["segs"][k] = (s, 0)
                if plan["arr"] is not None:
                    plan["arr"][k].ptr, plan["arr"][k].bytes = s.data_ptr(), s.numel() * s.element_size()
        for l in plan["others"]:
            l.reset_state_variables()
        if plan["arr"] is not None:
            _lib.check(_lib.lib().snn_fill_segments(plan["arr"], len(plan["segs"]),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "snn_fill_segments")
        else:
            for t, pat in plan["segs"]:
                t.zero_() if pat == 0 else t.view(torch.int32).fill_(pat - (1 << 32) if pat >> 31 else pat)
        for c in self.connections.values():
            c.reset_state_variables()
        before = _lib.epoch()
        for m in self.monitors.values():
            m.reset_state_variables()
        # a monitor emptying its recording is an assignment, but not one the descriptors depend on
        for key in ("_run_cache", "_reset_cache"):
            kept = self.__dict__.get(key)
            if kept is not None and kept["epoch"] == before:
                kept["epoch"] = _lib.epoch()

    def train(self, mode: bool = True) -> "torch.nn.Module":
        self.learning = mode
        return super().train(mode)

    # ------------------------------------------------------------------ pipelined runs
    def pipelined(self, depth: int = 64):
        """Context manager (an extension of the reference's API): inside it run() RETURNS WITHOUT WAITING for the device --

            with network.pipelined():
                for batch in inputs:                     # tensors already on the device
                    network.run({"X": batch}, time=250)
                    network.reset_state_variables()

        The host prepares and enqueues run k+1 while run k executes (a synchronous run() costs ~0.2 ms of host time per call at
        cfg2, during which the MI355X idles).  Results are the same bit for bit; what changes is WHEN two things happen:
          * the host generator (the stream DiehlAndCookNodes' one_spike arbitration draws from, rng.py) lives on the device between
            the runs of the section and is written back when the section is settled: at sync(), at the end of the `with` block,
            every `depth` runs, and before anything in this package reads the host generator (a synchronous run, a device encoder).
            Code of the CALLER that draws from torch's CPU generator inside the section must call network.sync() first;
          * the device status word is read at settlement.  An input the lean kernel form gives up on (SNN_ERR_RETRY) is repeated on
            the general form ON THE DEVICE (snn_run_desc.status2: the second attempt is enqueued behind every first one and returns
            at once where it is not needed), so that case stays exact; a SNN_ERR_TIMEOUT (the GPU was shared and a resident grid
            was not co-resident in time) cannot be repaired after later runs have been enqueued and raises SnnError at settlement
            -- use synchronous runs on a shared GPU."""
        import contextlib

        @contextlib.contextmanager
        def section():
            if self.__dict__.get("_pipe") is not None:
                raise RuntimeError("Network.pipelined() sections do not nest")
            from .. import rng
            pipe = self.__dict__["_pipe"] = _Pipeline(depth)
            rng._PENDING.append(self.sync)
            try:
                yield self
                self.sync()
            except BaseException:
                # the body raised: what has been enqueued still runs on the device -- settle it (so that the host generator stands where
                # those runs left it) without letting a second error hide the first
                try:
                    self.sync()
                except Exception:                          # noqa: BLE001
                    pass
                raise
            finally:
                rng._PENDING.remove(self.sync)
                self.__dict__["_pipe"] = None
                pipe.pending.clear()
        return section()

    def sync(self) -> None:
        """Settle the runs of an open pipelined() section: wait for them, check their status words, bring the host generator
        up to date.  A no-op outside a section / with nothing enqueued."""
        pipe = self.__dict__.get("_pipe")
        if pipe is None or not pipe.pending:
            return
        from ..rng import RNG_STATE_BYTES, words_to_torch_state
        n = len(pipe.pending)
        if pipe.stream is not None and pipe.stream != torch.cuda.current_stream(pipe.block.device):
            pipe.stream.synchronize()                      # the caller changed streams inside the section: the read-back below is ordered behind the CURRENT one only
        pipe.host.copy_(pipe.block)                        # blocking: everything enqueued so far has run
        st = pipe.status[:2 * n].cpu().numpy().reshape(n, 2)
        pipe.pending.clear()
        bad = None
        for k in range(n):
            s1, s2 = int(st[k, 0]), int(st[k, 1])
            if s1 == _lib.SNN_ERR_RETRY and s2 == 0:       # repeated on the general form, on the device
                self.__dict__["lean_retries"] = self.__dict__.get("lean_retries", 0) + 1
                self.__dict__["_lean_cooldown"] = 16
            elif (s1 != 0 or s2 != 0) and bad is None:
                bad = (k, s1, s2)
        if bad is not None:
            if pipe.enabled:
                torch.set_rng_state(pipe.host0)
            raise _lib.SnnError(f"pipelined run {bad[0] + 1} of {n} reported status {bad[1]} (second attempt: {bad[2]}); the runs enqueued "
                                "behind it have executed on the state it left, so the section cannot be repaired -- "
                                "SNN_ERR_TIMEOUT (-6) means the GPU was shared: use synchronous runs there")
        if pipe.enabled:
            # Between the first run of the batch and now the host generator was stale (its state lived on the device).  Whoever drew
            # from it meanwhile -- torch.rand, a host encoder called without this package's flush -- took numbers from the wrong
            # position, and writing the device image back would silently discard those draws: refuse instead of diverging.
            drew = not torch.equal(torch.get_rng_state(), pipe.host0)
            torch.set_rng_state(words_to_torch_state(pipe.host.numpy()[:RNG_STATE_BYTES // 4], pipe.host0))
            if drew:
                raise RuntimeError("Network.pipelined(): torch's CPU generator was used inside the section while its state lived on the device "
                                   "(draws taken from a stale position); call network.sync() before drawing from the host generator inside a section")

    def _run_pipelined(self, pipe, built, lib, stream, dev):
        """Enqueue one run of a pipelined() section (see there)."""
        from ..rng import RNG_STATE_BYTES, torch_state_to_words
        L, Cn, R, names = built["L"], built["Cn"], built["R"], built["names"]
        block, qbuf, host = built["gen_bufs"]
        draws = built["max_draws"] > 0
        cur_stream = torch.cuda.current_stream(dev)
        if pipe.pending and (len(pipe.pending) >= pipe.depth or draws != pipe.enabled or pipe.block is not block or cur_stream != pipe.stream):
            self.sync()                                    # (a batch lives on ONE stream: its runs hand the generator block from one to the next in stream order)
        if not pipe.pending:                               # first run of a batch: the host generator goes to the device
            img = host.numpy()
            img[:] = 0
            pipe.enabled, pipe.host0 = draws, None
            if draws:
                # another network's open section holds the host generator on ITS device block: settle it first, or both would
                # consume the same mt19937 segment and the later sync() would overwrite the earlier one's position
                from .. import rng
                for settle in list(rng._PENDING):
                    if settle != self.sync:
                        settle()
                pipe.host0 = torch.get_rng_state()
                img[:RNG_STATE_BYTES // 4] = torch_state_to_words(pipe.host0)
            block.copy_(host, non_blocking=True)           # (the previous settlement's blocking read-back ordered us behind it)
            if pipe.status is None or pipe.status.device != dev:
                pipe.status = torch.zeros(2 * pipe.depth, dtype=torch.int32, device=dev)
            else:
                pipe.status.zero_()
            pipe.block, pipe.host, pipe.stream = block, host, cur_stream
        k = len(pipe.pending)
        R.rng, R.qbuf = _dptr(block[:RNG_STATE_BYTES // 4]), _dptr(qbuf)
        R.cursor = C.c_void_p(block.data_ptr() + 632 * 4)
        R.status = C.c_void_p(pipe.status.data_ptr() + 8 * k)
        R.status2 = C.c_void_p(pipe.status.data_ptr() + 8 * k + 4)
        cool = self.__dict__.get("_lean_cooldown", 0)
        R.plan = 3 if cool > 0 else 0
        if cool > 0:
            self.__dict__["_lean_cooldown"] = cool - 1
        try:
            _lib.check(lib.snn_net_run_props(L, len(names), Cn, len(self.connections), built["Pn"], C.byref(R), stream), "snn_net_run")
        finally:
            R.status2 = None
        self.__dict__["last_plan"] = lib.snn_plan_name().decode()
        pipe.pending.append(self.last_plan)

    # ------------------------------------------------------------------ run
    def run(self, inputs: Dict[str, torch.Tensor], time: int, one_step=False, **kwargs) -> None:
        assert type(inputs) == dict, (
            "'inputs' must be a dict of names of layers (str) and relevant input tensors. "
            f"Got {type(inputs).__name__} instead.")
        clamps, unclamps = kwargs.get("clamp", {}) or {}, kwargs.get("unclamp", {}) or {}
        injects_v, masks = kwargs.get("injects_v", {}) or {}, kwargs.get("masks", {}) or {}
        self._normalise(inputs)
        dev = self._device()
        req = RunRequest.of(self, inputs, time, masks, injects_v, on_device=dev.type == "cuda")
        for err in self._preflight(req):                   # what any object of the network cannot run: before the run changes any state
            raise err
        if self.reward_fn is not None:
            kwargs["reward"] = self.reward_fn.compute(**kwargs)
        self._set_batch_size(req.B)
        T, B = req.T, self.batch_size
        if not req.on_device:
            # A network whose tensors live on the host: the plain-PyTorch step loop with the reference's semantics
            # (network/host_path.py).  Function, not speed -- the product is the MI355X path below; nothing is ever
            # silently moved between the two (a network on the GPU never falls back to this).
            if any(v.is_cuda for v in inputs.values()):
                raise _lib.SnnError("bindsnet_amd: the network is on the host but an input tensor is on the GPU: move the "
                                    "network with network.to('cuda')")
            if T <= 0:
                host_path.normalize(self)
                return
            host_path.run(self, inputs, T, one_step, kwargs)
            self.__dict__["last_plan"] = "host-torch"
            return
        if T <= 0:
            self._normalize_all()
            return
        # The descriptor arrays are kept from one call to the next: while nothing has been assigned to any object of the
        # network since they were built (_lib.epoch(), plus the in-place versions of the scalar parameter tensors they
        # were filled from) only the per-call pointers are rebound -- inputs, Input.s, monitor buffers.  Calls with
        # keyword arguments (clamp, masks, reward, ...) or one_step always build afresh.
        plain = not kwargs and not one_step and self.reward_fn is None and _DESC_CACHE
        built = self.__dict__.get("_run_cache") if plain else None
        if built is not None and not self._cache_valid(built, T, B, dev):
            built = None
        if built is None:
            built = self._build_descriptors(T, B, dev, one_step, kwargs, clamps, unclamps, injects_v, masks)
            self.__dict__["_run_cache"] = built if plain else None
        L, Cn, R, names = built["L"], built["Cn"], built["R"], built["names"]
        rasters, keep = self._bind_call(built, inputs, T, B, dev)
        gen_bufs, max_draws = built["gen_bufs"], built["max_draws"]
        lib = _lib.lib()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        # plan request of this run: automatic, unless the lean kernel form gave up on one of the last inputs (it is then
        # left alone for a while: an input it cannot finish costs a whole second run)
        pipe = self.__dict__.get("_pipe")
        if pipe is not None:
            self._run_pipelined(pipe, built, lib, stream, dev)
        cool = self.__dict__.get("_lean_cooldown", 0)
        R.plan = 3 if cool > 0 else 0
        if cool > 0 and pipe is None:
            self.__dict__["_lean_cooldown"] = cool - 1
        for attempt in (0, 1, 2) if pipe is None else ():
            with DeviceGenerator(dev, max_draws, gen_bufs) as ns:  # host generator <-> device, exact (rng.py)
                R.rng, R.qbuf = _dptr(ns.state), _dptr(ns.qbuf)
                R.cursor, R.status = _dptr(ns.cursor), _dptr(ns.status)
                _lib.check(lib.snn_net_run_props(L, len(names), Cn, len(self.connections), built["Pn"], C.byref(R), stream), "snn_net_run")
                self.__dict__["last_plan"] = lib.snn_plan_name().decode()
                # plans that hand spikes between workgroups report a failed hand-off (or a step the lean form does not
                # handle) through the status word: it is read back after EVERY such run, with or without one_spike
                ns.always_read = self.last_plan.startswith("dc2015-resident") or self.last_plan == "convpp-fused"
                status = ns.finish(check_status=attempt == 2)
            if status == 0:
                break
            # The kernel returned without touching any state tensor or the generator, so the same input is simply run
            # again: SNN_ERR_RETRY (lean form, unsupported step) -> the general resident kernel; SNN_ERR_TIMEOUT (the GPU
            # was shared and the grid was not co-resident in time) -> the one-launch-per-timestep plan, which cannot wait
            # on another workgroup.
            if status == _lib.SNN_ERR_RETRY:
                self.__dict__["lean_retries"] = self.__dict__.get("lean_retries", 0) + 1
                self.__dict__["_lean_cooldown"] = 16
                R.plan = 3
            else:
                self.__dict__["resident_retries"] = self.__dict__.get("resident_retries", 0) + 1
                R.plan = 2
        # (reached only behind a run that was enqueued whole: a run that raises leaves the layers' state and the windows undefined, as it
        #  does v and w)
        for k, conn in built["windows"]:               # every timestep overwrote the oldest slot of the ring
            win = conn.__dict__["_win"]
            win["head"] = (win["head"] + T) % win["ring"].shape[1]
        if not self.__dict__.get("_defer_norm", False):     # network.py:463-465 for the connections snn_net_run does not normalise itself
            for conn in self.connections.values():
                if conn._norm_by == "after" and conn.norm is not None:
                    conn.normalize()
        # Input.s aliases the last input slice, as in the reference (nodes.py:219)
        before = _lib.epoch()
        if self.learning:
            for k, rule in built["averages"]:          # every learning step moved the ring index of every term that ran
                rule._avg_advance(T)
        for i, name, layer, _ in built["inputs"]:
            layer.s = inputs[name][T - 1]
        for mon, key, buf in rasters:
            if isinstance(key, tuple):
                mon._append(key[0], key[1], buf)       # NetworkMonitor: (layer name, variable)
            else:
                mon._append(key, buf)
        self.__dict__["_keep"] = keep
        for kept in (built, self.__dict__.get("_reset_cache")):    # the assignments just made are this call's own
            if kept is not None and kept["epoch"] == before:
                kept["epoch"] = _lib.epoch()

    @staticmethod
    def _normalise(inputs) -> None:
        """network.py:329-339: inputs of shape [n] and [T, n] get their time and batch dimensions."""
        for key in inputs:
            if inputs[key].dim() == 1:
                inputs[key] = inputs[key].unsqueeze(0).unsqueeze(0)
            elif inputs[key].dim() == 2:
                inputs[key] = inputs[key].unsqueeze(1)

    def _set_batch_size(self, B: int) -> None:
        """network.py:340-353: the batch size follows the first input."""
        if B != self.batch_size:
            self.batch_size = B
            for l in self.layers.values():
                l.set_batch_size(B)
            for m in self.monitors.values():
                m.reset_state_variables()

    def _preflight(self, req: RunRequest):
        """Every reason against `req` in the order asked (some raised by the question itself): each connection, then its rule; each layer; the network's own."""
        def asked():
            for key, conn in self.connections.items():
                yield from conn._refusals(key, req)
                if req.learning:
                    yield from conn._rule()._refusals(key, req)
            for name, layer in self.layers.items():
                yield from layer._refusals(name, req)
            for m in self.monitors.values():               # a Monitor on a float16 / bfloat16 feature value: recordings are float32
                val = getattr(getattr(m, "obj", None), "value", None)
                if isinstance(val, torch.Tensor) and val.dtype in (torch.float16, torch.bfloat16):
                    yield NotImplementedError(f"bindsnet_amd: a Monitor on a {val.dtype} Weight.value is not supported")
            for name, layer in self.layers.items() if req.on_device else ():      # a real-valued input on the device (snnhip.h f17)
                x = req.inputs.get(name) if isinstance(layer, Input) else None
                if x is not None and x.is_floating_point() and x.dtype != torch.float32:
                    yield NotImplementedError(f"bindsnet_amd: inputs['{name}'] is {x.dtype}: a real-valued (analog) input must be float32 on "
                                              "the device; call .float() on it")
                elif name in req.analog and not req.readers(layer):
                    # (real values are defined by what reads them: without a Connection or Conv2dConnection the device has no use for them)
                    yield NotImplementedError(f"bindsnet_amd: inputs['{name}'] is {x.dtype}, but no Connection or Conv2dConnection reads the "
                                              f"Input layer '{name}': a real-valued (analog) input is accepted for those two classes; "
                                              "spike trains are uint8 or bool")
        return (err for err in asked() if err is not None)

    # ------------------------------------------------------------------ descriptors
    def _cache_valid(self, built, T, B, dev) -> bool:
        if built["epoch"] != _lib.epoch() or built["T"] != T or built["B"] != B or built["dev"] != dev:
            return False
        if built["n_objects"] != (len(self.layers), len(self.connections), len(self.monitors)):
            return False
        if built["defer_norm"] != bool(self.__dict__.get("_defer_norm", False)):
            return False
        for t, ver in built["scalars"]:               # parameter tensors changed in place (layer.thresh.fill_(...))
            if t._version != ver:
                return False
        for seq, vals in built["lists"]:              # list-valued parameters changed element-wise (rule.nu[0] = ...)
            if (seq._version if isinstance(seq, torch.Tensor) else tuple(seq)) != vals:
                return False
        for obj, attr, ptr in built["ptrs"]:          # tensors re-homed without an assignment (t.data = ..., set_(), resize_())
            t = getattr(obj, attr, None)
            if not isinstance(t, torch.Tensor) or t.data_ptr() != ptr:
                return False
        return True

    def _build_descriptors(self, T, B, dev, one_step, kwargs, clamps, unclamps, injects_v, masks):
        """Everything of the snn_net_run arguments that does not change from call to call."""
        from . import nodes as _nodes
        epoch0 = _lib.epoch()
        keep = []                                 # tensors that must outlive the asynchronous launch
        names = list(self.layers)
        index = {n: i for i, n in enumerate(names)}
        L = (_lib.LayerDesc * len(names))()
        dyn_inputs, dyn_layers = [], []
        records = []                              # (owner, attribute, [(monitor, key)]) per float32 tensor recorded through snn_run_desc.records
        max_draws = 0
        scalars = _nodes._SCALARS = []
        try:
            for i, name in enumerate(names):
                layer, d = self.layers[name], L[i]
                d.n = layer.n
                if isinstance(layer, Input):
                    d.kind = _lib.LAYER_INPUT
                    pv = {}                            # per-neuron tc_trace / additive trace_scale (nodes.py:96-107 broadcast them)
                    layer._trace_fields(d.p.lif, pv)
                    layer._fill_pv(d, pv, keep)
                    d.x = _dptr(layer.x) if layer.traces else None
                    wanted, traced = [], []            # (monitor, key) pairs recording this layer's spikes / its trace
                    for m in self.monitors.values():
                        if isinstance(m, Monitor) and m.obj is layer:
                            for var in m.state_vars:
                                if var != "s" and var not in layer._recordable():
                                    raise NotImplementedError("bindsnet_amd: Input layers can only be monitored for 's'"
                                                              + (" and 'x'" if layer.traces else " (and 'x' with traces=True)"))
                                (wanted if var == "s" else traced).append((m, var))
                        elif isinstance(m, NetworkMonitor):
                            got = m._wanted()
                            if (name, "s") in got:
                                wanted.append((m, (name, "s")))
                            if (name, "x") in got and layer.traces:
                                traced.append((m, (name, "x")))
                    if traced:
                        self._check_recorded(layer, "x", B * layer.n, dev)
                        records.append((layer, "x", traced))
                    dyn_inputs.append((i, name, layer, wanted))
                    continue
                if type(layer)._describe is Nodes._describe:
                    layer._describe(d, keep, scalars)             # (raises: a layer type outside the accelerated path)
                self._check_state(layer, B, dev)
                requests = self._monitor_requests(layer, name)
                for var in dict.fromkeys(v for _, _, v in requests if v not in ("s", "v")):      # x, theta, refrac_count, i: one buffer per tensor
                    self._check_recorded(layer, var, layer.n if var == "theta" else B * layer.n, dev)
                    records.append((layer, var, [(m, key) for m, key, v in requests if v == var]))
                requests = [r for r in requests if r[2] in ("s", "v")]
                cur = self._scratch("cur_" + name, (B, layer.n), torch.float32, dev)
                d.v, d.s, d.current = _dptr(layer.v), _dptr(layer.s), _dptr(cur)
                d.refrac = _dptr(layer.refrac_count) if "refrac_count" in layer._STATE else None
                d.x = _dptr(layer.x) if layer.traces else None
                dyn_layers.append((i, layer, requests))
                # clamp / unclamp / injects_v (network.py:395-429): [n] masks or values, or one slice per timestep
                for key, table in (("clamp", clamps), ("unclamp", unclamps)):
                    m = table.get(name)
                    if m is not None:
                        m = host_path.clamp_mask(m, layer.n).to(dev)      # boolean masks, or neuron INDICES like supervised_mnist.py:201-207
                        per_step = m.dim() >= 2
                        if m.numel() != (T if per_step else 1) * layer.n and not (per_step and m.shape[0] >= T and m[0].numel() == layer.n):
                            raise ValueError(f"{key}['{name}'] must have {layer.n} entries (optionally one row per timestep)")
                        m = (m[:T] if per_step else m).ne(0).to(torch.uint8).contiguous()
                        keep.append(m)
                        setattr(d, key, _dptr(m))
                        setattr(d, key + "_per_step", int(per_step))
                inj = injects_v.get(name)
                if inj is not None:
                    inj = torch.as_tensor(inj).to(dev, torch.float32)
                    per_step = inj.dim() >= 2
                    one = inj[0] if per_step else inj
                    if one.numel() not in (layer.n, B * layer.n) or (per_step and inj.shape[0] < T):
                        raise ValueError(f"injects_v['{name}'] must have {layer.n} (or batch x {layer.n}) entries, optionally per timestep")
                    inj = (inj[:T] if per_step else inj).contiguous()
                    keep.append(inj)
                    d.inject_v, d.inject_per_step, d.inject_len = _dptr(inj), int(per_step), one.numel()
                max_draws = max(max_draws, layer._describe(d, keep, scalars))      # the class's own part: kind, parameters, extra state
        except BaseException:
            _nodes._SCALARS = None
            raise

        try:           # ONE guard from here to the end of the collection: whatever raises in between must not leave a stale collector behind
            for table, what in ((clamps, "clamp"), (unclamps, "unclamp"), (injects_v, "injects_v")):
                for lname in table:
                    if lname not in self.layers or isinstance(self.layers[lname], Input):
                        raise NotImplementedError(f"bindsnet_amd: {what}['{lname}'] must name a non-Input layer of the network")
            Cn = (_lib.ConnDesc * max(1, len(self.connections)))()
            Pn = (_lib.ConnProp * max(1, len(self.connections)))()      # snn_conn_prop, index for index
            lists, dyn_conns, described, windows, averages = [], [], [], [], []
            for k, ((src, dst), conn) in enumerate(self.connections.items()):
                described += self._fill_conn(Cn[k], conn, self._source_index(names, index, src, conn), index[dst], B, dev, keep, kwargs)   # (the collector stays on: clamp bounds are read through _f() as well)
                if hasattr(conn, "_describe_prop"):
                    described += conn._describe_prop(Pn[k], Cn[k], B, dev, self._scratch)
                if self.__dict__.get("_defer_norm", False):    # parallel.sharded_run normalises the MERGED weights itself
                    Cn[k].has_norm = 0
                wanted = self._conn_monitor_requests(conn, (src, dst))
                if wanted:
                    dyn_conns.append((k, conn, wanted))
                traced = self._activity_requests(conn)
                if traced:                             # (the buffer itself: MulticompartmentConnection._describe, traces=True)
                    records.append((conn, "activity", traced))
                if Cn[k].window:
                    windows.append((k, conn))
                if Cn[k].avg_k:                        # average_update: the ring indices are per-call values, the rings' addresses are watched
                    averages.append((k, conn._rule()))
                    described += [(conn._rule(), ring) for ring, _, _ in conn._rule()._RINGS]
                nu = getattr(conn._rule(), "nu", None)
                if isinstance(nu, torch.Tensor):
                    lists.append((nu, nu._version))
                elif isinstance(nu, (list, tuple)):
                    lists.append((nu, tuple(nu)))
                mask = host_path._mask_of(conn, masks.get((src, dst)))
                if mask is not None:
                    if not conn._takes_mask:
                        raise NotImplementedError("bindsnet_amd: weight masks are supported on dense connections")
                    m = torch.as_tensor(mask).to(dev).ne(0).to(torch.uint8).contiguous()
                    if m.numel() != conn.w.numel():
                        raise ValueError(f"mask of connection {(src, dst)} must have the shape of its weights")
                    keep.append(m)
                    Cn[k].mask = _dptr(m)
        except BaseException:
            _nodes._SCALARS = None
            raise

        _nodes._SCALARS = None
        if any(Cn[k].pipe_n and _lib.MCC_OP_MUL_DRAW in list(Cn[k].pipe_kind)[:Cn[k].pipe_n] for k in range(len(self.connections))):
            max_draws = max(max_draws, 1)         # a Probability draws from the host generator: it goes to the device for the run (rng.py)
        # every tensor whose ADDRESS went into the descriptors: `t.data = other`, set_() or resize_() re-home a tensor
        # without any attribute assignment, so the kept arrays are only valid while these still are where they were
        ptrs = []
        for layer in self.layers.values():
            for attr in layer._watched() + [k for k in _lib.PERVEC if isinstance(getattr(layer, k, None), torch.Tensor) and getattr(layer, k).numel() > 1]:
                ptrs.append((layer, attr, getattr(layer, attr).data_ptr()))
            if not isinstance(layer, Input) and isinstance(getattr(layer, "s", None), torch.Tensor):
                ptrs.append((layer, "s", layer.s.data_ptr()))
        ptrs += [(obj, attr, getattr(obj, attr).data_ptr()) for obj, attr in described]     # what the connections' _describe wrote
        R = _lib.RunDesc()
        R.B, R.T, R.dt, R.learning = B, T, float(self.dt), int(self.learning)
        R.one_step = int(bool(one_step))                  # network.py:388-393 (generic plan)
        rec_arr = (_lib.RecordSegment * len(records))() if records else None
        for k, (owner, attr, _) in enumerate(records):    # the sources stay where they are (`ptrs` watches them); _bind_call gives every call fresh recordings
            t = getattr(owner, attr)
            rec_arr[k].src, rec_arr[k].bytes = t.data_ptr(), 4 * t.numel()
        need = int(_lib.lib().snn_net_workspace_bytes(L, len(names), Cn, len(self.connections), C.byref(R)))
        if need:
            ws = self.__dict__.get("_workspace")
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self.__dict__["_workspace"] = torch.empty(need, dtype=torch.uint8, device=dev)
                self.__dict__["_ws_state"] = (C.c_ulonglong * 2)()       # snn_run_desc.host_state: what the library knows about the workspace's content
            R.workspace, R.workspace_bytes = _dptr(ws), need
            R.host_state = C.cast(self.__dict__.setdefault("_ws_state", (C.c_ulonglong * 2)()), C.c_void_p)
        pool = self.__dict__.setdefault("_scratch_pool", {})
        if "rng_host" not in pool:
            pool["rng_host"] = torch.zeros(640, dtype=torch.int32).pin_memory()
        gen_bufs = (self._scratch("rng_block", (640,), torch.int32, dev),
                    self._scratch("rng_qbuf", (max(max_draws, 1),), torch.float32, dev), pool["rng_host"])
        # (assignments made while building -- a state tensor re-created by _check_state, a rule's lazily allocated
        #  memory -- belong to this build: the descriptors already point at the new objects)
        return {"L": L, "Cn": Cn, "Pn": Pn, "R": R, "names": names, "keep": keep, "inputs": dyn_inputs, "layers": dyn_layers, "conns": dyn_conns, "windows": windows, "averages": averages, "records": records, "rec_arr": rec_arr,
                "max_draws": max_draws, "gen_bufs": gen_bufs, "T": T, "B": B, "dev": dev, "scalars": scalars,
                "lists": lists, "epoch": _lib.epoch(), "n_objects": (len(self.layers), len(self.connections), len(self.monitors)),
                "epoch0": epoch0, "defer_norm": bool(self.__dict__.get("_defer_norm", False)), "ptrs": ptrs}

    def _bind_call(self, built, inputs, T, B, dev):
        """The per-call part of the descriptors: input spike trains, Input.s (it aliases the previous call's last
        slice), freshly allocated monitor buffers."""
        L = built["L"]
        keep = list(built["keep"])
        rasters = []                              # (monitor, key, tensor)
        for i, name, layer, wanted in built["inputs"]:
            if name not in inputs:
                raise NotImplementedError(f"bindsnet_amd: Input layer '{name}' needs an entry in `inputs`")
            x = inputs[name]
            if x.shape[0] < T:
                raise ValueError(f"inputs['{name}'] has {x.shape[0]} timesteps, run() needs {T}")
            if x.dtype not in (torch.uint8, torch.bool, torch.float32):
                raise NotImplementedError("bindsnet_amd: input spike trains must be uint8 or bool, or float32 for a real-valued "
                                          f"(analog) input (got {x.dtype}); encoders produce uint8")
            analog = is_analog(layer, x)                   # (what it may drive: the readers' _refusals, before the run began)
            x = x.to(dev).contiguous()
            if x.numel() != x.shape[0] * B * layer.n:
                raise ValueError(f"inputs['{name}'] has shape {tuple(x.shape)}, expected [T, {B}, {layer.n}]")
            if analog:                                 # a real-valued Input (snnhip.h f17): the float twins of ext_spikes / s / raster_s
                x = x.float()                          # (a byte train behind a float `s` left by an analog run: promoted, exact)
                entry = layer.s
                if entry.numel() != B * layer.n or entry.device != dev:
                    entry = torch.zeros(B, layer.n, dtype=torch.float32, device=dev)
                entry = entry.float().contiguous()     # (a byte `s` left by a spike run: by value, as compute()'s s.float())
                keep += [x, entry]
                L[i].ext_spikes, L[i].s, L[i].raster_s = None, None, None
                L[i].ext_real, L[i].s_real = _dptr(x), _dptr(entry)
                if wanted:
                    xcopy = torch.empty_like(x[:T])
                    L[i].raster_real = _dptr(xcopy)
                    rasters += [(m, key, xcopy.view(T, B, *layer.shape)) for m, key in wanted]
                else:
                    L[i].raster_real = None
                inputs[name] = x
                continue
            L[i].ext_real, L[i].s_real, L[i].raster_real = None, None, None
            entry = layer.s
            if entry.dtype not in (torch.uint8, torch.bool) or entry.numel() != B * layer.n or entry.device != dev:
                entry = torch.zeros(B, layer.n, dtype=torch.uint8, device=dev)
            entry = entry.contiguous()
            keep += [x, entry]
            L[i].ext_spikes, L[i].s = _dptr(x), _dptr(entry)
            if wanted:                             # the raster of an input layer is a COPY of its input, like Monitor.record's
                # clone (monitors.py:94-111): the caller may refill its buffer in place.  The library makes the copy (snn_layer_desc.raster_s
                # of an INPUT layer): one device copy behind the plan, or -- third-generation D&C form -- by the launch's producer workgroups
                xcopy = torch.empty_like(x[:T])
                L[i].raster_s = _dptr(xcopy)
                rasters += [(m, key, xcopy.view(T, B, *layer.shape)) for m, key in wanted]
            else:
                L[i].raster_s = None
            inputs[name] = x
        for i, layer, requests in built["layers"]:
            # an entry of `inputs` for a non-Input layer is an external CURRENT (network.py:386-392): slice t is added to
            # the layer's summed input behind the connections' contributions (generic plan)
            ext = inputs.get(built["names"][i])
            if ext is not None:
                if ext.shape[0] < T or ext[0].numel() != B * layer.n:
                    raise ValueError(f"inputs['{built['names'][i]}'] has shape {tuple(ext.shape)}, expected [T >= {T}, {B}, {layer.n}]")
                ext = ext[:T].to(dev, torch.float32).contiguous()
                keep.append(ext)
                L[i].ext_current = _dptr(ext)
            else:
                L[i].ext_current = None
            mon_s = mon_v = None
            for m, key, var in requests:
                if var == "s":
                    if mon_s is None:              # bool like layer.s; the node kernels store a 0/1 byte for EVERY
                        # (step, sample, neuron), so the buffer needs no initialisation
                        mon_s = torch.empty(T, B, *layer.shape, dtype=torch.bool, device=dev)
                    rasters.append((m, key, mon_s))
                else:
                    if mon_v is None:
                        mon_v = torch.empty(T, B, *layer.shape, device=dev)
                    rasters.append((m, key, mon_v))
            L[i].raster_s, L[i].raster_v = _dptr(mon_s), _dptr(mon_v)
        for k, conn in built["windows"]:           # a connection into a CSRM layer: its ring and where the oldest entry stands now
            win = conn._window_ring(B, dev)
            built["Cn"][k].win_ring, built["Cn"][k].win_head = _dptr(win["ring"]), win["head"]
        for k, rule in built["averages"]:          # an averaged rule: where its ring indices stand now (they moved with every learning step since)
            idx = rule._avg_indices()
            built["Cn"][k].avg_i0, built["Cn"][k].avg_i1 = idx[0], idx[-1]
        for k, conn, wanted in built["conns"]:    # weights at the end of every timestep (monitors.py:94-111, 222-262)
            mon_w = torch.empty(T, *self._monitored_weights(conn).shape, device=dev)
            built["Cn"][k].raster_w = _dptr(mon_w)
            rasters += [(m, key, mon_w) for m, key in wanted]
        # float state at the end of every timestep (monitors.py:94-111): one [T, *shape] buffer per tensor, shared by its monitors
        # and new for every call -- what an earlier get() handed out is never written again
        R, rec_arr = built["R"], built["rec_arr"]
        for k, (owner, attr, wanted) in enumerate(built["records"]):
            buf = torch.empty(T, *getattr(owner, attr).shape, dtype=torch.float32, device=dev)
            rec_arr[k].dst = buf.data_ptr()
            rasters += [(m, key, buf) for m, key in wanted]
        R.records, R.n_records = (rec_arr, len(built["records"])) if rec_arr is not None else (None, 0)
        return rasters, keep

    # ------------------------------------------------------------------ helpers
    def _scratch(self, key, shape, dtype, dev):
        """Persistent device scratch: the same addresses run after run avoid allocator traffic."""
        pool = self.__dict__.setdefault("_scratch_pool", {})
        t = pool.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev:
            t = pool[key] = torch.empty(shape, dtype=dtype, device=dev)
        return t

    def _normalize_all(self):
        if self._device().type != "cuda":          # a network on the host: plain PyTorch (network/host_path.py)
            host_path.normalize(self)
            return
        for c in self.connections.values():
            c.normalize()

    def _device(self) -> torch.device:
        for l in self.layers.values():
            if hasattr(l, "v"):
                return l.v.device
        for l in self.layers.values():
            return l.s.device
        return torch.device("cpu")

    def _source_index(self, names, index, src, conn) -> int:
        """The layer a connection reads: its own `source` object, as in the reference (network.py:227), whatever name the
        connection was filed under -- ann_to_snn files a connection behind a skipped child under a name no layer has."""
        if self.layers.get(src) is conn.source:
            return index[src]
        for i, name in enumerate(names):
            if self.layers[name] is conn.source:
                return i
        raise KeyError(f"the source layer of connection {(src,)} is not a layer of the network")

    @staticmethod
    def _check_state(layer, B, dev):
        for nm in layer._STATE + (("x",) if layer.traces else ()):
            t = getattr(layer, nm)
            if t.device != dev or t.dtype != torch.float32 or t.numel() != B * layer.n or not t.is_contiguous():
                raise ValueError(f"layer state '{nm}' must be a contiguous float32 [{B}, {layer.n}] tensor on {dev}")
        if layer.s.dtype not in (torch.bool, torch.uint8) or layer.s.numel() != B * layer.n or layer.s.device != dev \
                or not layer.s.is_contiguous():
            layer.s = torch.zeros(B, *layer.shape, dtype=torch.bool, device=dev)

    def _monitor_requests(self, layer, name):
        """(monitor, key handed back to its _append, variable) for every monitor recording this layer."""
        requests = []
        for m in self.monitors.values():
            if isinstance(m, NetworkMonitor):
                requests += [(m, (l, v), v) for l, v in m._wanted() if l == name]
            elif isinstance(m, Monitor):
                if m.obj is layer:
                    requests += [(m, v, v) for v in m.state_vars]
                elif not isinstance(m.obj, Nodes) and not any(m.obj is c for c in self.connections.values()) and self._feature_owner(m.obj) is None:
                    raise NotImplementedError("bindsnet_amd: monitors on objects other than the network's layers and "
                                              "connections (features, ...) are not supported")
        for m, key, var in requests:
            if var != "s" and not (var == "v" and "v" in layer._STATE) and var not in layer._recordable():
                supported = ["s"] + (["v"] if "v" in layer._STATE else []) + list(layer._recordable())
                raise NotImplementedError(f"bindsnet_amd: monitoring '{var}' of {type(layer).__name__} is outside the accelerated "
                                          "path (supported on this layer: " + ", ".join(f"'{v}'" for v in supported)
                                          + "; 'x' with traces=True; 'theta', 'refrac_count' and 'i' where the class keeps them)")
        return requests

    @staticmethod
    def _check_recorded(owner, attr, numel, dev):
        """A tensor a state monitor records: what snn_record_segments copies, float32 words in place."""
        t = getattr(owner, attr, None)
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or t.numel() != numel or not t.is_contiguous():
            raise ValueError(f"monitored state '{attr}' of {type(owner).__name__} must be a contiguous float32 tensor of {numel} elements on {dev}")

    @staticmethod
    def _records_activity(m, conn) -> bool:
        """Whether `m` is a Monitor of nothing but the `activity` of `conn`, a MulticompartmentConnection(traces=True)."""
        return isinstance(m, Monitor) and m.obj is conn and getattr(conn, "traces", False) and list(m.state_vars) == ["activity"]

    def _activity_requests(self, conn):
        """(monitor, key handed back to its _append) for every Monitor recording the `activity` of a traces=True connection."""
        return [(m, "activity") for m in self.monitors.values() if self._records_activity(m, conn)]

    def _feature_owner(self, obj):
        """The MulticompartmentConnection whose pipeline holds the feature `obj` (a Monitor on a Weight records its `value`), or None."""
        for conn in self.connections.values():
            if any(obj is f for f in getattr(conn, "pipeline", ())):
                return conn
        return None

    def _conn_monitor_requests(self, conn, cname):
        """(monitor, key handed back to its _append) for every monitor recording this connection's weights."""
        requests = []
        for m in self.monitors.values():
            if isinstance(m, NetworkMonitor):
                requests += [(m, (c, v)) for c, v in m._wanted_conns() if c == cname]
            elif self._records_activity(m, conn):
                continue                               # (_activity_requests: recorded through snn_run_desc.records)
            elif isinstance(m, Monitor) and m.obj is conn:
                if list(m.state_vars) != ["w"] or not hasattr(conn, "w"):
                    raise NotImplementedError(f"bindsnet_amd: monitoring {list(m.state_vars)} of {type(conn).__name__} is outside "
                                              "the accelerated path (supported on connections: 'w'; 'activity' alone on a "
                                              "MulticompartmentConnection with traces=True)")
                requests.append((m, "w"))
            elif isinstance(m, Monitor) and any(m.obj is f for f in getattr(conn, "pipeline", ())):
                # a Monitor on a feature (monitors.py:94-111 records any attribute): the `value` of the Weight the rule refers to --
                # what the connection hands to snn_net_run as `w` -- is copied at the end of every timestep like a connection's `w`
                if list(m.state_vars) != ["value"] or m.obj is not conn._learned():
                    raise NotImplementedError(f"bindsnet_amd: monitoring {list(m.state_vars)} of the feature '{m.obj.name}' is outside the "
                                              "accelerated path (supported: 'value' of the Weight the rule or the norm refers to)")
                requests.append((m, "value"))
        w = self._monitored_weights(conn) if requests else None
        if requests and (w.dtype != torch.float32 or not w.is_contiguous()):
            raise NotImplementedError("bindsnet_amd: monitored connection weights must be contiguous float32")
        return requests

    @staticmethod
    def _monitored_weights(conn):
        """The tensor a weight monitor of this connection records: `w`, or the learned Weight's value of a MulticompartmentConnection."""
        return conn._learned().value if hasattr(conn, "pipeline") else conn.w

    def _fill_conn(self, d, conn, src, dst, B, dev, keep, kwargs):
        """One snn_conn_desc: the connection describes itself, then its rule does.  Returns the connection's (owner, attribute)
        pairs of the tensors whose addresses `d` now holds."""
        if not hasattr(conn, "_describe"):
            raise NotImplementedError(f"bindsnet_amd: connection type {type(conn).__name__} is not supported")
        d.src, d.dst, d.rule, d.wdecay = src, dst, _lib.RULE_NONE, 1.0
        described = conn._describe(d, B, dev, self._scratch)
        rule = conn._rule()
        if not hasattr(rule, "_describe"):
            raise NotImplementedError(f"bindsnet_amd: rule {type(rule).__name__} is not supported")
        if rule._rule_code != _lib.RULE_NONE:
            rule._describe(d, conn, B, dev, keep, kwargs)
        elif getattr(rule, "weight_decay", 1.0) != 1.0 and self.learning:
            # the reference's NoOp.update still decays w every step (learning.py:87-104); not on the accelerated path
            raise NotImplementedError("bindsnet_amd: weight_decay on a connection without a learning rule is not supported")
        return described
