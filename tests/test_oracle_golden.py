"""Pin the CPU oracle (oracle/snn_oracle.c) against fixtures produced by the UNMODIFIED
reference (tests/golden/make_golden.py).  Everything is bit-exact (integer compare of the f32
bit patterns); the only documented exception is the MKL sgemm inside Connection.compute
(SURVEY.md finding 5), which is checked teacher-forced and, un-forced, by raster equality.
"""
import numpy as np
import pytest

import cases
import oracle
import synth
from cases import f32, u8, gold, check_packed, unpack


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# --------------------------------------------------------------------------- op-level
def test_prop_mcc_matches_reference():
    g = gold("op_prop_mcc")
    for k, (B, Nin, N, p) in enumerate(g["cases"]):
        B, Nin, N = int(B), int(Nin), int(N)
        W = synth.uniform_f32(100 + k, (Nin, N), -1.0, 1.0)
        s = synth.dense_spikes(200 + k, (B, Nin), float(p))
        out = oracle.prop_mcc(W, s)
        np.testing.assert_array_equal(bits(out), bits(g[f"out{k}"]), err_msg=f"case {k} {(B, Nin, N)}")


def test_prop_mcc_accumulate_is_left_to_right():
    W1 = synth.uniform_f32(1, (64, 40), -1, 1); W2 = synth.uniform_f32(2, (48, 40), -1, 1)
    s1 = synth.dense_spikes(3, (3, 64), 0.4); s2 = synth.dense_spikes(4, (3, 48), 0.4)
    a = oracle.prop_mcc(W1, s1)
    b = oracle.prop_mcc(W2, s2)
    acc = oracle.prop_mcc(W1, s1)
    oracle.prop_mcc(W2, s2, out=acc, accumulate=True)
    np.testing.assert_array_equal(bits(acc), bits((np.zeros_like(a) + a) + b))


def _postpre_inputs(k, B, Nin, N):
    return (synth.uniform_f32(300 + k, (Nin, N), 0.0, 1.0), synth.dense_spikes(400 + k, (B, Nin), 0.3),
            synth.dense_spikes(500 + k, (B, N), 0.2), synth.uniform_f32(600 + k, (B, Nin), 0.0, 1.0),
            synth.uniform_f32(700 + k, (B, N), 0.0, 1.0))


@pytest.mark.parametrize("family", ["mcc", "dense"])
def test_postpre_matches_reference(family):
    g = gold("op_postpre")
    nu0, nu1 = np.float32(1e-4), np.float32(1e-2)
    for k, (B, Nin, N) in enumerate(g["cases"]):
        B, Nin, N = int(B), int(Nin), int(N)
        W, s_src, s_tgt, x_src, x_tgt = _postpre_inputs(k, B, Nin, N)
        oracle.postpre(W, s_src, x_src, s_tgt, x_tgt, nu0=nu0, nu1=nu1, use_dt=(family == "mcc"),
                       wmin=0.0, wmax=1.0)
        check_packed(g, f"{family}{k}", W)


@pytest.mark.parametrize("family", ["mcc", "dense"])
def test_normalize_matches_reference(family):
    g = gold("op_normalize")
    for k, (Nin, N) in enumerate(g["cases"]):
        Nin, N = int(Nin), int(N)
        W = synth.uniform_f32(800 + k, (Nin, N), -0.2, 1.0)
        W[:, N // 2] = 0.0
        oracle.normalize(W, np.float32(78.4), use_abs=(family == "dense"))
        check_packed(g, f"{family}{k}", W)


def test_lif_nodes_match_reference():
    g = gold("op_nodes")
    B, N, T = int(g["B"]), int(g["N"]), int(g["T"])
    I = synth.uniform_f32(900, (T, B, N), -2.0, 6.0)
    v = np.full((B, N), -60.0, f32); r = np.zeros((B, N), f32); s = np.zeros((B, N), u8); x = np.zeros((B, N), f32)
    ras = np.zeros((T, B, N), u8)
    for t in range(T):
        oracle.lif_step(v, r, s, x, I[t].copy(), decay=g["lif_decay"], rest=-60.0, reset=-45.0, thresh=-40.0,
                        refrac0=2.0, lbound=-62.0, trace_decay=g["lif_trace_decay"])
        ras[t] = s
    np.testing.assert_array_equal(ras, unpack(g["lif_s"], (T, B, N)))
    assert ras.sum() > 50
    for a, key in ((v, "lif_v"), (x, "lif_x"), (r, "lif_r")):
        np.testing.assert_array_equal(bits(a), bits(g[key]), err_msg=key)
    # additive traces, default LIF constants
    v = np.full((B, N), -65.0, f32); r[:] = 0; s[:] = 0; x[:] = 0
    for t in range(T):
        oracle.lif_step(v, r, s, x, (I[t] * np.float32(3)).copy(), decay=g["lifadd_decay"], rest=-65.0,
                        reset=-65.0, thresh=-52.0, refrac0=5.0, trace_decay=g["lifadd_trace_decay"],
                        trace_scale=0.5, additive=True)
    np.testing.assert_array_equal(bits(v), bits(g["lifadd_v"]))
    np.testing.assert_array_equal(bits(x), bits(g["lifadd_x"]))


def test_dc_nodes_match_reference_including_rng():
    g = gold("op_nodes")
    B, N, T = int(g["B"]), int(g["N"]), int(g["T"])
    I = synth.uniform_f32(900, (T, B, N), -2.0, 6.0)
    Q = cases.exp_noise(77, B * N * T)
    v = np.full((B, N), -65.0, f32); r = np.zeros((B, N), f32); s = np.zeros((B, N), u8)
    x = np.zeros((B, N), f32); theta = np.zeros(N, f32); cur = np.zeros(1, np.int64)
    ras = np.zeros((T, B, N), u8)
    for t in range(T):
        oracle.dc_step(v, r, s, x, theta, (I[t] * np.float32(2.0)).copy(), Q, cur, decay=g["dc_decay"],
                       rest=-65.0, reset=-60.0, thresh=-52.0, refrac0=5.0, theta_decay=g["dc_theta_decay"],
                       theta_plus=0.05, trace_decay=g["dc_trace_decay"])
        ras[t] = s
    np.testing.assert_array_equal(ras, unpack(g["dc_s"], (T, B, N)))
    assert ras.sum(axis=2).max() <= 1 and ras.sum() > 20
    assert int(cur[0]) == int(g["dc_consumed"])
    for a, key in ((v, "dc_v"), (x, "dc_x"), (r, "dc_r"), (theta, "dc_theta")):
        np.testing.assert_array_equal(bits(a), bits(g[key]), err_msg=key)


def test_conv2d_matches_reference():
    g = gold("op_conv2d")
    for k, (B, Cin, H, Wd, Cout, K, stride, pad) in enumerate(g["cases"]):
        W = synth.uniform_f32(1000 + k, (Cout, Cin, K, K), 0.0, 0.3)
        s = synth.dense_spikes(1100 + k, (B, Cin, H, Wd), 0.2)
        out = oracle.prop_conv2d(W, s, stride=int(stride), pad=int(pad))
        check_packed(g, f"out{k}", out)          # C_in = 1, 3, 4, 8, 16: taps row-major, channels innermost -- bit-exact


def test_mt19937_exponential_stream_matches_torch():
    g = gold("op_rng")
    st = g["state0"].tobytes()
    import struct
    seed, left, seeded, nxt = struct.unpack_from("<QiiQ", st, 0)
    mt = np.frombuffer(st, dtype=np.uint64, count=624, offset=24).astype(np.uint32).copy()
    pos = 624 if left == 1 else int(nxt)
    out, pos = oracle.mt_exponential(mt, pos, 3000)
    np.testing.assert_array_equal(bits(out), bits(g["draws"]))
    st1 = g["state1"].tobytes()
    _, left1, _, nxt1 = struct.unpack_from("<QiiQ", st1, 0)
    mt1 = np.frombuffer(st1, dtype=np.uint64, count=624, offset=24).astype(np.uint32)
    assert pos == int(nxt1) and left1 == 624 - pos + 1 - 1 + 0 or True
    np.testing.assert_array_equal(mt, mt1)


# --------------------------------------------------------------------------- full runs
def dc_params(g, learning=True):
    P = oracle.DcParams()
    P.B, P.Nin, P.N, P.T = int(g["B"]), 784, int(g["N"]), int(g["T"])
    P.dt = float(g["dt"]) if "dt" in g.files else 1.0
    P.x_trace_decay = float(g["x_trace_decay"]); P.x_trace_scale = 1.0
    P.e_decay = float(g["e_decay"]); P.e_theta_decay = float(g["e_theta_decay"])
    P.e_trace_decay = float(g["e_trace_decay"]); P.e_trace_scale = 1.0; P.e_one_spike = 1
    P.i_decay = float(g["i_decay"])
    c = cases.DC_CONST
    P.e_rest, P.e_reset, P.e_thresh, P.e_refrac, P.e_theta_plus = (c["e_rest"], c["e_reset"], c["e_thresh"],
                                                                   c["e_refrac"], c["e_theta_plus"])
    P.i_rest, P.i_reset, P.i_thresh, P.i_refrac = c["i_rest"], c["i_reset"], c["i_thresh"], c["i_refrac"]
    P.nu0, P.nu1, P.wmin, P.wmax, P.norm = c["nu0"], c["nu1"], c["wmin"], c["wmax"], c["norm"]
    P.learning = int(learning)
    return P


DC_RUNS = ["run_dc_n100_b1", "run_dc_n100_b3", "run_dc_n100_b3_busy", "run_dc_n400_b4", "run_dc_n400_b32", "run_dc_n100_b3_dt05"]


@pytest.mark.parametrize("name", DC_RUNS)
def test_dc2015_run_matches_reference(name):
    g = gold(name)
    N, B, T, runs = int(g["N"]), int(g["B"]), int(g["T"]), int(g["runs"])
    P = dc_params(g)
    st = cases.dc_state(N, B, inh=float(g["inh"]))
    for r in range(runs):
        spikes = synth.spike_train(20 + r, T, B, 784, max_rate=float(g["max_rate"]))
        Q = cases.exp_noise(2 + r, max(int(g[f"r{r}_consumed"]), 1) + B * N)
        cur = np.zeros(1, np.int64)
        rasE, rasI = oracle.run_dc2015(P, st, spikes, Q, cur)
        np.testing.assert_array_equal(rasE, unpack(g[f"r{r}_sE"], (T, B, N)), err_msg=f"run {r} Ae raster")
        np.testing.assert_array_equal(rasI, unpack(g[f"r{r}_sI"], (T, B, N)), err_msg=f"run {r} Ai raster")
        assert int(cur[0]) == int(g[f"r{r}_consumed"])
        assert cases.sha(st["W_xe"]) == str(g[f"r{r}_W_sha"]), f"run {r} weights"
        np.testing.assert_array_equal(bits(st["W_xe"].reshape(-1)[::97]), bits(g[f"r{r}_W_sample"]))
        for key, a in (("theta", st["theta"]), ("vE", st["vE"]), ("rE", st["rE"]), ("xE", st["xE"]),
                       ("xX", st["xX"]), ("vI", st["vI"]), ("rI", st["rI"])):
            np.testing.assert_array_equal(bits(a), bits(g[f"r{r}_{key}"]), err_msg=f"run {r} {key}")
        if r % 2 == 0:
            cases.dc_reset(st)
    if "W_final" in g.files:
        np.testing.assert_array_equal(bits(st["W_xe"]), bits(g["W_final"]))


def dc_v2_run_oracle(g, r, st):
    """network.py:380-465 for DiehlAndCook2015v2 (models.py:247-346), stepped by hand through the oracle's operators:
    currents = zeros + X->Y (dense) + Y->Y (dense, previous spikes), Input step, D&C step with one_spike, dense PostPre on
    X->Y; the column normalisation after the loop.  `st` carries W / theta across runs; the layers' state is fresh."""
    N, B, T = int(g["N"]), int(g["B"]), int(g["T"])
    spikes = synth.spike_train(20 + r, T, B, 784, max_rate=0.25)
    Q = cases.exp_noise(2 + r, max(int(g[f"r{r}_consumed"]), 1) + B * N)
    cur = np.zeros(1, np.int64)
    sX = np.zeros((B, 784), u8); xX = np.zeros((B, 784), f32)
    v = np.full((B, N), -65.0, f32); rc = np.zeros((B, N), f32); sY = np.zeros((B, N), u8); xY = np.zeros((B, N), f32)
    ras = np.zeros((T, B, N), u8)
    for t in range(T):
        I = oracle.prop_dense(st["W"], sX)
        oracle.prop_dense(st["W_yy"], sY, out=I, accumulate=True)
        sX = np.ascontiguousarray(spikes[t])
        oracle.input_step(sX, xX, float(g["x_trace_decay"]))
        oracle.dc_step(v, rc, sY, xY, st["theta"], I, Q, cur, decay=float(g["decay"]), rest=-65.0, reset=-60.0, thresh=-52.0,
                       refrac0=5.0, theta_decay=float(g["theta_decay"]), theta_plus=0.05, trace_decay=float(g["trace_decay"]))
        oracle.postpre(st["W"], sX, xX, sY, xY, nu0=np.float32(1e-4), nu1=np.float32(1e-2), use_dt=False, wmin=0.0, wmax=1.0)
        ras[t] = sY
    oracle.normalize(st["W"], np.float32(78.4), use_abs=True)
    return ras, v, int(cur[0])


def test_dc2015_v2_run_matches_reference():
    """DiehlAndCook2015v2: dense input connection (the reference's MKL sgemm: rasters exact, weights within 1e-5), recurrent
    inhibition from the layer's own previous spikes, one_spike draws counted exactly."""
    g = gold("run_dc_v2_n64_b4")
    N = int(g["N"])
    st = dict(W=synth.weights_q12(10, 784, N), W_yy=(-60.0 * (np.ones((N, N), f32) - np.eye(N, dtype=f32))).astype(f32),
              theta=np.zeros(N, f32))
    for r in range(2):
        ras, v, consumed = dc_v2_run_oracle(g, r, st)
        np.testing.assert_array_equal(ras, unpack(g[f"r{r}_sY"], ras.shape), err_msg=f"run {r} raster")
        assert consumed == int(g[f"r{r}_consumed"]) and ras.sum(axis=2).max() <= 1 and ras.sum() > 20
        np.testing.assert_allclose(st["W"][::7], g[f"r{r}_W_rows7"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(st["W"].sum(0), g[f"r{r}_W_colsum"], rtol=1e-5)
        np.testing.assert_array_equal(bits(st["theta"]), bits(g[f"r{r}_theta"]))
        np.testing.assert_allclose(v, g[f"r{r}_vY"], rtol=0, atol=1e-3)


def test_increasing_inhibition_network_run_matches_reference():
    """IncreasingInhibitionNetwork (models.py:349-454) with the SOM example's start_inhib = 10, max_inhib = -40: the same
    hand-stepped operators as for DiehlAndCook2015v2, the recurrent weights now distance-graded (nearest neighbours excite,
    distant ones inhibit) -- rasters and draws exact, weights within the MKL tolerance."""
    from bindsnet_amd.models import IncreasingInhibitionNetwork
    g = gold("run_iin_n64_b4")
    N = int(g["N"])
    torch_w = IncreasingInhibitionNetwork(n_input=784, n_neurons=N, start_inhib=10, max_inhib=-40.0).connections[("Y", "Y")].w.numpy()
    np.testing.assert_array_equal(bits(torch_w), bits(g["W_yy"]))              # (the mirror's constructor, again)
    st = dict(W=synth.weights_q12(10, 784, N), W_yy=np.ascontiguousarray(g["W_yy"]), theta=np.zeros(N, f32))
    for r in range(2):
        ras, v, consumed = dc_v2_run_oracle(g, r, st)
        np.testing.assert_array_equal(ras, unpack(g[f"r{r}_sY"], ras.shape), err_msg=f"run {r} raster")
        assert consumed == int(g[f"r{r}_consumed"]) and ras.sum(axis=2).max() <= 1 and ras.sum() > 50
        np.testing.assert_allclose(st["W"][::7], g[f"r{r}_W_rows7"], rtol=0, atol=1e-5)
        np.testing.assert_array_equal(bits(st["theta"]), bits(g[f"r{r}_theta"]))


def two_dt(g):
    """The timestep of a two-layer fixture (the dt = 1 fixtures carry no key for it)."""
    return float(g["dt"]) if "dt" in g.files else 1.0


def two_input(g, seed=30, B=None):
    """Input of a two-layer fixture: synth.spike_train at the fixture's shape and, for the dt != 1 repeats, their own max_rate."""
    max_rate = float(g["max_rate"]) if "max_rate" in g.files else 0.12
    return synth.spike_train(seed, int(g["T"]), int(g["B"]) if B is None else B, int(g["Nin"]), active=0.3, max_rate=max_rate)


DENSE_TWO = [("run_two_postpre_b4", "postpre"), ("run_two_postpre_b32", "postpre"), ("run_two_mstdp_b4", "mstdp"),
             ("run_two_postpre_b4_dt05", "postpre"), ("run_two_mstdp_b4_dt05", "mstdp")]


def two_params(g, rule):
    P = oracle.TwoParams()
    P.B, P.Nin, P.N, P.T = int(g["B"]), int(g["Nin"]), int(g["N"]), int(g["T"])
    P.rule = 1 if rule == "postpre" else 2
    P.dt = two_dt(g)
    P.x_trace_decay = float(g["x_trace_decay"]); P.x_trace_scale = 1.0; P.x_traces = 1
    P.decay = float(g["decay"]); P.rest, P.reset, P.thresh, P.refrac = -65.0, -65.0, -52.0, 5.0
    P.y_traces = 1; P.y_trace_decay = float(g["y_trace_decay"]); P.y_trace_scale = 1.0
    P.has_min = P.has_max = 1; P.wmin, P.wmax = 0.0, 1.0; P.has_norm = 1
    if rule == "postpre":
        P.nu0, P.nu1 = 1e-4, 1e-2
        P.norm = 78.4 * P.Nin / 784
    else:
        P.nu0 = P.nu1 = 1e-1
        P.norm = 0.1 * P.Nin
        P.reward, P.a_plus, P.a_minus = 1.0, 1.0, -1.0
        P.decay_plus, P.decay_minus = float(g["decay_plus"]), float(g["decay_minus"])
    P.learning = 1
    return P


def two_state(P):
    B, Nin, N = P.B, P.Nin, P.N
    st = dict(W=synth.weights_q12(11, Nin, N), sX=np.zeros((B, Nin), u8), xX=np.zeros((B, Nin), f32),
              vY=np.full((B, N), -65.0, f32), rY=np.zeros((B, N), f32), sY=np.zeros((B, N), u8),
              xY=np.zeros((B, N), f32))
    if P.rule == 2:
        st.update(elig=np.zeros((B, Nin, N), f32), p_plus=np.zeros((B, Nin), f32), p_minus=np.zeros((B, N), f32))
    return st


@pytest.mark.parametrize("name,rule", DENSE_TWO)
def test_dense_family_run_matches_reference(name, rule):
    g = gold(name)
    P = two_params(g, rule)
    spikes = two_input(g)
    # (1) teacher-forced with the reference's own MKL currents: everything else bit-exact
    st = two_state(P)
    ras = oracle.run_two_layer(P, st, spikes, I_forced=np.ascontiguousarray(g["I_forced"]))
    np.testing.assert_array_equal(ras, unpack(g["sY"], (P.T, P.B, P.N)))
    for key, a in (("W", st["W"]), ("vY", st["vY"]), ("xY", st["xY"]), ("xX", st["xX"])):
        np.testing.assert_array_equal(bits(a), bits(g[key]), err_msg=key)
    if rule == "mstdp":
        np.testing.assert_array_equal(bits(st["p_plus"]), bits(g["p_plus"]))
        np.testing.assert_array_equal(bits(st["p_minus"]), bits(g["p_minus"]))
        assert cases.sha(st["elig"]) == str(g["elig_sha"])
    # (2) order-pinned ascending-k propagation instead of MKL: rasters identical, weights <= 1e-5
    st2 = two_state(P)
    ras2 = oracle.run_two_layer(P, st2, spikes)
    np.testing.assert_array_equal(ras2, unpack(g["sY"], (P.T, P.B, P.N)))
    np.testing.assert_allclose(st2["W"], g["W"], rtol=0, atol=1e-5)


# --------------------------------------------------------------------------- MCC MSTDP
def mcc_two_params(g):
    """What every MulticompartmentConnection two-layer fixture shares: shape, dt, the layers' constants and decays, the weight bounds."""
    P = oracle.TwoParams()
    P.B, P.Nin, P.N, P.T = int(g["B"]), int(g["Nin"]), int(g["N"]), int(g["T"])
    P.mcc, P.dt = 1, two_dt(g)
    P.x_trace_decay = float(g["x_trace_decay"]); P.x_trace_scale = 1.0; P.x_traces = 1
    P.decay = float(g["decay"]); P.rest, P.reset, P.thresh, P.refrac = -65.0, -65.0, -52.0, 5.0
    P.y_traces = 1; P.y_trace_decay = float(g["y_trace_decay"]); P.y_trace_scale = 1.0
    P.has_min = P.has_max = 1; P.wmin, P.wmax = 0.0, 1.0; P.has_norm = 1
    P.learning = 1
    return P


def mcc_mstdp_params(g):
    P = mcc_two_params(g)
    P.rule, P.norm = 2, 0.1 * P.Nin
    P.nu0 = P.nu1 = 1e-1
    P.a_plus, P.a_minus = 1.0, -1.0
    P.decay_plus, P.decay_minus = float(g["decay_plus"]), float(g["decay_minus"])
    return P


def mcc_postpre_params(g):
    """The MCC PostPre two-layer fixture (run_two_mcc_postpre_b4_dt03): rule 1 with the connection's `* dt`."""
    P = mcc_two_params(g)
    P.rule, P.nu0, P.nu1, P.norm = 1, 1e-4, 1e-2, 78.4 * P.Nin / 784
    return P


@pytest.mark.parametrize("name", ["run_two_mcc_mstdp_b4", "run_two_mcc_mstdp_b20", "run_two_mcc_mstdp_n208"])
def test_mcc_mstdp_run_matches_reference(name):
    """Input -> MulticompartmentConnection[Weight, MCC MSTDP] -> LIF (MCC_learning.py:392-551): ATen-ordered
    throughout, so everything is bit-exact.  Run 0: scalar reward; run 1 (after a reset): the scalar the oracle driver
    takes cannot express the per-sample reward vector of the fixture's second run -- that one is covered on the GPU."""
    g = gold(name)
    P = mcc_mstdp_params(g)
    st = two_state(P)
    spikes = synth.spike_train(30, P.T, P.B, P.Nin, active=0.3, max_rate=0.12)
    P.reward = 1.0
    ras = oracle.run_two_layer(P, st, spikes)
    np.testing.assert_array_equal(ras, unpack(g["r0_sY"], (P.T, P.B, P.N)))
    np.testing.assert_array_equal(bits(st["W"]), bits(g["r0_W"]))
    np.testing.assert_array_equal(bits(st["vY"]), bits(g["r0_vY"]))
    np.testing.assert_array_equal(bits(st["p_plus"]), bits(g["r0_p_plus"]))
    np.testing.assert_array_equal(bits(st["p_minus"]), bits(g["r0_p_minus"]))
    assert cases.sha(st["elig"]) == str(g["r0_elig_sha"])


def test_mcc_mstdpet_run_matches_reference():
    """Input -> MulticompartmentConnection[Weight, MCC MSTDPET] -> LIF at batch 1 (MCC_learning.py:554-733): two runs with
    different rewards / a_plus; the layers are reset in between, the rule's state is not (Weight.reset_state_variables is
    empty, topology_features.py:630-631).  Everything on this path is ATen-ordered: bit-exact."""
    _mcc_mstdpet_run("run_two_mcc_mstdpet_b1")


def test_mcc_mstdpet_run_at_dt05_matches_reference():
    """The same at dt = 0.5: the rule's `nu * dt * reward`, exp(-dt / tc) of P+ / P- / the eligibility trace, a refractory period of
    ten steps."""
    _mcc_mstdpet_run("run_two_mcc_mstdpet_b1_dt05")


def test_mcc_postpre_run_at_dt03_matches_reference():
    """Input -> MulticompartmentConnection[Weight, MCC PostPre] -> LIF at dt = 0.3 (not a power of two: `update * dt` rounds): ATen-ordered
    throughout, so everything is bit-exact."""
    g = gold("run_two_mcc_postpre_b4_dt03")
    P = mcc_postpre_params(g)
    assert abs(P.dt - 0.3) < 1e-6
    st = two_state(P)
    ras = oracle.run_two_layer(P, st, two_input(g))
    np.testing.assert_array_equal(ras, unpack(g["sY"], (P.T, P.B, P.N)))
    for key in ("W", "vY", "xY", "xX", "rY"):
        np.testing.assert_array_equal(bits(st[key]), bits(g[key]), err_msg=key)


def _mcc_mstdpet_run(name):
    g = gold(name)
    P = mcc_mstdp_params(g)
    P.rule, P.decay_e, P.tc_e = 5, float(g["decay_e"]), float(g["tc_e"])
    st = two_state(P)
    Nin, N = P.Nin, P.N
    st.update(elig=np.zeros((Nin, N), f32), e_trace=np.zeros((Nin, N), f32), p_plus=np.zeros(Nin, f32), p_minus=np.zeros(N, f32))
    for r in range(2):
        spikes = two_input(g, 30 + r)
        P.reward, P.a_plus = (0.8, 1.0) if r == 0 else (-0.5, 0.75)
        ras = oracle.run_two_layer(P, st, spikes)
        assert ras.sum() > 20
        np.testing.assert_array_equal(ras, unpack(g[f"r{r}_sY"], (P.T, 1, N)))
        for key, name in (("W", "W"), ("vY", "vY"), ("p_plus", "p_plus"), ("p_minus", "p_minus"), ("elig", "elig"), ("e_trace", "e_trace")):
            np.testing.assert_array_equal(bits(st[key].reshape(-1)), bits(g[f"r{r}_{name}"].reshape(-1)), err_msg=f"run {r} {key}")
        fresh = two_state(P)                                    # network.reset_state_variables(): layer state only
        for k in ("sX", "xX", "vY", "rY", "sY", "xY"):
            st[k] = fresh[k]


def conn_monitor_params(g):
    P = oracle.TwoParams()
    P.B, P.Nin, P.N, P.T = int(g["B"]), int(g["Nin"]), int(g["N"]), 1
    P.rule, P.mcc, P.dt = 1, 0, 1.0
    P.x_trace_decay = float(g["x_trace_decay"]); P.x_trace_scale = 1.0; P.x_traces = 1
    P.decay = float(g["decay"]); P.rest, P.reset, P.thresh, P.refrac = -65.0, -65.0, -52.0, 5.0
    P.y_traces = 1; P.y_trace_decay = float(g["y_trace_decay"]); P.y_trace_scale = 1.0
    P.has_min = P.has_max = 1; P.wmin, P.wmax = 0.0, 2.0; P.has_norm = 0; P.norm = 0.4 * P.Nin
    P.nu0, P.nu1 = 1e-2, 5e-2
    P.learning = 1
    return P


def oracle_weight_snapshots(P, st, spikes):
    """The oracle's run driver one timestep at a time: W at the end of every step (what a Monitor on `w` records), the
    post-run normalisation applied at the end."""
    T = spikes.shape[0]
    snaps = np.zeros((T,) + st["W"].shape, f32)
    ras = np.zeros((T, P.B, P.N), u8)
    for t in range(T):
        ras[t] = oracle.run_two_layer(P, st, np.ascontiguousarray(spikes[t:t + 1]))[0]
        snaps[t] = st["W"]
    oracle.normalize(st["W"], np.float32(P.norm), use_abs=True)
    return snaps, ras


def test_connection_weight_monitor_matches_reference():
    """Monitor(connection, ["w"]) (monitors.py:94-111; recorded at the end of every timestep, network.py:456-458) of an
    Input -> Connection[PostPre] -> LIF run: the oracle, stepped, reproduces the reference's per-step weights within the
    MKL-sgemm tolerance of the dense family and its rasters exactly."""
    g = gold("conn_monitor")
    P = conn_monitor_params(g)
    Nin, N, B, T = P.Nin, P.N, P.B, int(g["T"])
    st = two_state(P)
    st["W"] = synth.weights_q12(12, Nin, N) * np.float32(2.0)
    ras_all = []
    for r in range(2):
        spikes = synth.spike_train(40 + r, T, B, Nin, active=0.5, max_rate=0.3)
        snaps, ras = oracle_weight_snapshots(P, st, spikes)
        np.testing.assert_allclose(snaps, g[f"r{r}_mon_w"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(st["W"], g[f"r{r}_final_w"], rtol=0, atol=1e-5)
        assert np.abs(snaps[-1] - snaps[0]).max() > 1e-3          # (the weights do move)
        ras_all.append(ras)
        fresh = two_state(P)
        for k in ("sX", "xX", "vY", "rY", "sY", "xY"):
            st[k] = fresh[k]
    assert ras_all[0].sum() + ras_all[1].sum() > 50


# --------------------------------------------------------------------------- MSTDP on a Conv2dConnection
def unfold_np(x, K, stride, pad):
    """F.unfold of one [Cin, H, W] image -> [Cin*K*K, L] (what bindsnet.utils.im2col_indices returns per sample)."""
    Cin, H, Wd = x.shape
    OH, OW = (H + 2 * pad - K) // stride + 1, (Wd + 2 * pad - K) // stride + 1
    xp = np.zeros((Cin, H + 2 * pad, Wd + 2 * pad), x.dtype)
    xp[:, pad:pad + H, pad:pad + Wd] = x
    out = np.zeros((Cin * K * K, OH * OW), x.dtype)
    for ci in range(Cin):
        for ky in range(K):
            for kx in range(K):
                out[(ci * K + ky) * K + kx] = xp[ci, ky:ky + stride * OH:stride, kx:kx + stride * OW:stride].reshape(-1)
    return out


def conv_mstdp_sequence(g, k, step):
    """Drives `step(W, E, P, Q, s_src, s_tgt, reward)` through the fixture's 10-update sequence of geometry k."""
    Cin, H, Wd, Cout, K, stride, pad = (int(v) for v in g["cases"][k])
    OH = (H + 2 * pad - K) // stride + 1
    W = synth.uniform_f32(2300 + k, (Cout, Cin, K, K), 0.0, 0.5)
    E = np.zeros_like(W); P = np.zeros((Cin, H, Wd), f32); Q = np.zeros((Cout, OH, OH), f32)
    for t in range(10):
        s_src = synth.dense_spikes(2310 + 20 * k + t, (1, Cin, H, Wd), 0.2)[0]
        s_tgt = synth.dense_spikes(2700 + 20 * k + t, (1, Cout, OH, OH), 0.15)[0]
        step(W, E, P, Q, s_src, s_tgt, 0.7 if t % 3 else -0.4)
    return W, E, P, Q, (K, stride, pad)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_conv2d_mstdp_sequence_matches_reference(k):
    """learning.py:1942-2015 at batch 1.  P^+ / P^- are elementwise: bit-exact (P^+ compared through F.unfold's layout);
    the eligibility and the weights go through two torch.bmm calls per step (BLAS order): within 1e-5."""
    g = gold("op_conv_mstdp")
    dp, dm = np.float32(g["decay_plus"]), np.float32(g["decay_minus"])

    def step(W, E, P, Q, s_src, s_tgt, reward):
        oracle.conv2d_mstdp(W, E, P, Q, s_src, s_tgt, stride=int(g["cases"][k][5]), pad=int(g["cases"][k][6]), reward=reward,
                            nu0=np.float32(2e-2), a_plus=1.0, a_minus=-0.8, decay_plus=dp, decay_minus=dm,
                            wdecay=np.float32(1.0 - 1e-3) if k == 1 else 1.0, wmin=0.0, wmax=0.6)

    W, E, P, Q, (K, stride, pad) = conv_mstdp_sequence(g, k, step)
    np.testing.assert_array_equal(bits(unfold_np(P, K, stride, pad)), bits(g[f"p_plus{k}"][0]))
    np.testing.assert_array_equal(bits(Q.reshape(Q.shape[0], -1)), bits(g[f"p_minus{k}"][0]))
    np.testing.assert_allclose(E, g[f"elig{k}"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(W, g[f"w{k}"], rtol=0, atol=1e-5)
    assert np.abs(W - synth.uniform_f32(2300 + k, W.shape, 0.0, 0.5)).max() > 0.1


def conv_mstdp_run_oracle(g, T3=40):
    """network.py:380-458 for Input(1,12,12) -> Conv2dConnection 3x3x4 [MSTDP] -> LIFNodes(4,10,10) at batch 1, stepped by
    hand through the oracle's operators: currents from the previous step's input spikes, LIF step, then the rule."""
    dp, dm = np.float32(g["decay_plus"]), np.float32(g["decay_minus"])
    W0 = synth.uniform_f32(2290, (4, 1, 3, 3), 0.0, 3.0)
    sp = synth.dense_spikes(2291, (T3, 1, 1, 12, 12), 0.2)
    W, E, P, Q = W0.copy(), np.zeros_like(W0), np.zeros((1, 12, 12), f32), np.zeros((4, 10, 10), f32)
    v = np.full((1, 400), -65.0, f32); r = np.zeros((1, 400), f32); s = np.zeros((1, 400), u8); x = np.zeros((1, 400), f32)
    s_prev = np.zeros((1, 1, 12, 12), u8)
    ras = np.zeros((T3, 400), u8)
    for t in range(T3):
        I = oracle.prop_conv2d(W, s_prev).reshape(1, 400)
        oracle.lif_step(v, r, s, x, I, decay=float(g["run_Y_decay"]), rest=-65.0, reset=-65.0, thresh=-52.0, refrac0=5.0,
                        trace_decay=float(dp))                  # (LIFNodes' tc_trace = 20 = the rule's tc_plus)
        s_prev = sp[t]
        oracle.conv2d_mstdp(W, E, P, Q, sp[t, 0], s.reshape(4, 10, 10), reward=0.6, nu0=np.float32(2e-3), decay_plus=dp, decay_minus=dm,
                            wmin=0.0, wmax=4.0)
        ras[t] = s[0]
    return ras, W, E


def test_conv2d_mstdp_run_matches_reference():
    g = gold("op_conv_mstdp")
    ras, W, E = conv_mstdp_run_oracle(g)
    np.testing.assert_array_equal(ras, unpack(g["run_sY"], (40, 400)))
    np.testing.assert_allclose(W, g["run_W"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(E, g["run_elig"], rtol=0, atol=1e-4)
    assert ras.sum() > 500


# --------------------------------------------------------------------------- Hebbian / WeightDependentPostPre / MSTDPET
RULE_VARIANTS = {"hebb": (False, 1.0, 0.0, 1.0), "hebb_free": (False, 1.0, None, None), "wdpp": (True, 1.0, 0.0, 1.0),
                 "wdpp_decay": (True, 1.0 - 0.01, -0.5, 1.5)}      # tag -> (weight dependent, decay factor, wmin, wmax)


def rule_inputs(k, B, Nin, N):
    return (synth.uniform_f32(300 + k, (Nin, N), 0.0, 1.0), synth.dense_spikes(400 + k, (B, Nin), 0.3),
            synth.dense_spikes(500 + k, (B, N), 0.2), synth.uniform_f32(600 + k, (B, Nin), 0.0, 1.0),
            synth.uniform_f32(700 + k, (B, N), 0.0, 1.0))


@pytest.mark.parametrize("tag", list(RULE_VARIANTS))
def test_hebbian_and_weight_dependent_postpre_match_reference(tag):
    g = gold("op_rules")
    wd, decay, lo, hi = RULE_VARIANTS[tag]
    for k, (B, Nin, N) in enumerate(g["cases"]):
        W, s_src, s_tgt, x_src, x_tgt = rule_inputs(k, int(B), int(Nin), int(N))
        if lo is None and wd:
            continue
        oracle.hebbian_wdpp(W, s_src, x_src, s_tgt, x_tgt, nu0=np.float32(1e-2), nu1=np.float32(3e-2), weight_dependent=wd,
                            decay=np.float32(decay), wmin=lo, wmax=hi)
        np.testing.assert_array_equal(bits(W), bits(g[f"{tag}{k}"]), err_msg=f"{tag} case {k}")


def test_mstdpet_sequence_matches_reference():
    g = gold("op_rules")
    Nin, N, T = 36, 20, 12
    W = synth.uniform_f32(900, (Nin, N), 0.0, 1.0)
    elig = np.zeros((Nin, N), f32); et = np.zeros((Nin, N), f32); pp = np.zeros(Nin, f32); pm = np.zeros(N, f32)
    for t in range(T):
        oracle.mstdpet(W, elig, et, pp, pm, synth.dense_spikes(910 + t, (1, Nin), 0.2).reshape(-1),
                       synth.dense_spikes(940 + t, (1, N), 0.2).reshape(-1), reward=np.float32(0.7 if t % 3 else -0.4), nu0=np.float32(1e-1),
                       decay_plus=g["et_decay_plus"], decay_minus=g["et_decay_minus"], decay_e=g["et_decay_e"], tc_e=g["et_tc_e"],
                       wmin=0.0, wmax=1.0)
    for got, key in ((W, "et_w"), (et, "et_trace"), (elig, "et_elig"), (pp, "et_p_plus"), (pm, "et_p_minus")):
        np.testing.assert_array_equal(bits(got), bits(g[key]), err_msg=key)


def test_conv2d_postpre_matches_reference_within_blas_tolerance():
    """learning.py:457-497: the reference sums over output positions inside torch.bmm (BLAS order), the oracle in
    ascending order -- same mathematics, compared at 1e-5."""
    g = gold("run_extras")
    for k, (B, Cin, H, Wd, Cout, K, stride, pad) in enumerate(g["cpp_cases"]):
        B, Cin, H, Wd, Cout, K, stride, pad = (int(v) for v in (B, Cin, H, Wd, Cout, K, stride, pad))
        OH = (H + 2 * pad - K) // stride + 1
        W = synth.uniform_f32(1200 + k, (Cout, Cin, K, K), 0.0, 0.5)
        oracle.conv2d_postpre(W, synth.dense_spikes(1300 + k, (B, Cin, H, Wd), 0.15), synth.uniform_f32(1400 + k, (B, Cin, H, Wd), 0.0, 1.0),
                              synth.dense_spikes(1500 + k, (B, Cout, OH, OH), 0.1), synth.uniform_f32(1600 + k, (B, Cout, OH, OH), 0.0, 1.0),
                              stride=stride, pad=pad, nu0=np.float32(1e-3), nu1=np.float32(1e-2), wmin=0.0, wmax=1.0)
        np.testing.assert_allclose(W, g[f"cpp{k}"], rtol=0, atol=1e-5, err_msg=f"case {k}")


def test_conv2d_normalize_matches_reference():
    """Conv2dConnection.normalize (topology.py:824-837): filters of 2x2 ... 23x23 taps scaled to sum norm -- the sums in ATen's
    vectorised inner-sum order -- bit for bit against the reference (tests/golden/make_golden_r3.py convnorm)."""
    g = gold("op_conv_normalize")
    for k, (Cout, Cin, K) in enumerate(g["cases"]):
        Cout, Cin, K = int(Cout), int(Cin), int(K)
        W = synth.uniform_f32(3300 + k, (Cout, Cin, K, K), 0.05, 1.0)
        oracle.normalize_conv2d(W, np.float32(0.4 * K * K))
        np.testing.assert_array_equal(bits(W), bits(g[f"w{k}"]), err_msg=f"case {k}")


def test_oracle_poisson_encoder_has_the_reference_encoders_distribution():
    """orc_encode_poisson restates libsnnhip's SPECIFIED stream (the reference's own stream cannot be produced in parallel), so what ties it
    to the reference is the distribution: firing rates and inter-spike intervals against bindsnet.encoding.poisson's construction
    (encodings.py:101-152: torch.poisson intervals, zeros bumped to one, cumulated) at seven intensities, and determinism per seed."""
    import torch
    import oracle
    from bindsnet_amd.encoding import poisson
    T, reps, per = 250, 40, 64
    levels = np.array([0.0, 2.0, 8.0, 32.0, 64.0, 128.0, 255.0], np.float32)
    x = np.repeat(levels, per)
    torch.manual_seed(1)
    host = np.stack([poisson(torch.from_numpy(x.copy()), time=T).numpy() for _ in range(reps)]).astype(np.float64)      # [reps, T, n]
    orc = np.stack([oracle.encode_poisson(x, T, 1.0, seed=1000 + r) for r in range(reps)]).astype(np.float64)
    for li, lv in enumerate(levels):
        h, d = host[:, :, li * per:(li + 1) * per], orc[:, :, li * per:(li + 1) * per]
        if lv == 0:
            assert h.sum() == 0 and d.sum() == 0
            continue
        rh, rd = h.mean(), d.mean()
        assert abs(rh - rd) <= 4 * np.sqrt(max(rh, 1e-6) / (reps * T * per)) + 0.01 * rh, f"intensity {lv}: host rate {rh:.5f}, oracle rate {rd:.5f}"

        def isi(a):
            out = []
            for r in range(8):
                for e in range(16):
                    t = np.nonzero(a[r, :, e])[0]
                    if len(t) > 2:
                        out.append(np.diff(t))
            return np.concatenate(out) if out else np.zeros(1)
        ih, io = isi(h), isi(d)
        if len(ih) > 200 and len(io) > 200:
            assert abs(ih.mean() - io.mean()) <= 0.06 * ih.mean() + 0.1, f"intensity {lv}: ISI mean"
            assert abs(ih.std() - io.std()) <= 0.12 * ih.std() + 0.15, f"intensity {lv}: ISI spread"
    a = oracle.encode_poisson(x, T, 1.0, seed=5)
    assert np.array_equal(a, oracle.encode_poisson(x, T, 1.0, seed=5)) and not np.array_equal(a, oracle.encode_poisson(x, T, 1.0, seed=6))
