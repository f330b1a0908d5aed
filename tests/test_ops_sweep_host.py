"""The checker of tests/test_gpu_ops_sweep.py, checked first: at the shapes of tests/ops_sweep_cases.py

* oracle.normalize against the reference's own expression in torch on the CPU and against host_path._normalize_columns, both
  `use_abs`, real-valued weights with one all-zero column, bit for bit;
* oracle.prop_mcc against (s.float().unsqueeze(2) * W).sum(1), every spike pattern, bit for bit;
  (torch pinned to one thread: the serial order, tests/test_aten_sum_threads.py)
* the oracle's Diehl&Cook winner on hand-built ties against torch.argmax(mask / q);
* the tables themselves: every value of every thinned factor kept, the tile widths the plasticity rows were chosen for;
* that the reference ALONE shows the activity the device tests rely on: spikes and neurons on `lbound`, rows that cross and rows
  that do not, weights on both bounds and weights that moved, the zero column kept.

The remaining ops keep the oracle as tests/test_oracle_golden.py pins it.  The run_* helpers are the oracle sides of the device tests."""
import numpy as np
import pytest
import torch

import oracle
import ops_sweep_cases as SC

f32, u8 = np.float32, np.uint8


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture
def one_thread():
    n0 = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n0)


# ---------------------------------------------------------------------------------------------------------------- the tables
def test_thinned_products_keep_every_value_and_the_tiles_are_the_launchers():
    props, dcs = SC.prop_shapes(), SC.dc_shapes()
    assert {s[0] for s in props} == set(SC.PROP_B) and {s[1] for s in props} == set(SC.PROP_NIN) and {s[2] for s in props} == set(SC.PROP_N)
    assert {s[0] for s in dcs} == set(SC.DC_B) | {300} and {s[1] for s in dcs} == set(SC.DC_N)
    for B, TJ in SC.PLASTICITY_B.items():
        assert SC.plasticity_tile(B) == TJ, B
    # the conv rows are on the side of each limit their comments name
    lds = [SC.conv_lds_bytes(r) for r in SC.CONV_ROWS]
    assert lds[0] == (64000, 5, 69120) and lds[1] == (44800, 5, 56320)
    assert lds[2][1] == 0 and lds[3][1] == 0 and lds[4][1] == 257 and all(l[0] <= 64 * 1024 for l in lds)
    assert all(r[1] <= 16 for r in SC.CONV_ROWS)
    assert SC.MSTDP_CAP[0] * (SC.MSTDP_CAP[1] + SC.MSTDP_CAP[2]) > 2048 * 256 and SC.MSTDPET_CAP[0] * SC.MSTDPET_CAP[1] > 4096 * 256


# ---------------------------------------------------------------------------------------------------------------- normalize
def normalize_cases():
    """(Nin, N, zero the column): every shape with column N // 2 zeroed; a single column also as it is drawn (its zeroed form has no sum)."""
    return [(Nin, N, True) for Nin, N in SC.NORMALIZE_SHAPES] + [(Nin, N, False) for Nin, N in SC.NORMALIZE_SHAPES if N == 1]


def run_normalize_oracle(Nin, N, use_abs, zero_column=True):
    W0 = SC.normalize_weights(Nin, N, zero_column)
    W = W0.copy()
    oracle.normalize(W, SC.NORM, use_abs)
    if zero_column:
        assert (W[:, N // 2] == 0).all()                     # the zero column stayed zero
    if N > 1 or not zero_column:
        assert (W != W0).any()                               # and another one changed
    return W0, W


@pytest.mark.parametrize("use_abs", [False, True])
@pytest.mark.parametrize("Nin,N,zero", normalize_cases())
def test_oracle_normalize_is_the_references_expression(Nin, N, zero, use_abs, one_thread):
    from bindsnet_amd.network.host_path import _normalize_columns
    W0, got = run_normalize_oracle(Nin, N, use_abs, zero)
    w = torch.from_numpy(W0.copy())
    s = w.abs().sum(0) if use_abs else w.sum(0)             # topology.py:383-392 / topology_features.py:250-266
    s[s == 0] = 1.0
    w *= SC.NORM / s
    assert np.array_equal(bits(got), bits(w.numpy())), int((bits(got) != bits(w.numpy())).sum())
    h = torch.from_numpy(W0.copy())
    _normalize_columns(h, SC.NORM, use_abs)
    assert np.array_equal(bits(got), bits(h.numpy()))


# ---------------------------------------------------------------------------------------------------------------- propagation
@pytest.mark.parametrize("B,Nin,N", SC.prop_shapes())
def test_oracle_prop_mcc_is_the_references_sum(B, Nin, N, one_thread):
    W, _, _, patterns = SC.prop_inputs(B, Nin, N)
    assert [n for n, _ in patterns] == [p for p in SC.PROP_PATTERNS if p != "at1023" or Nin > 1023]
    for name, s in patterns:
        want = (torch.from_numpy(s).float().unsqueeze(2) * torch.from_numpy(W)).sum(1).numpy()
        got = oracle.prop_mcc(W, s)
        assert np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).sum()))
    assert set(np.unique(patterns[-1][1])) <= {0, 1, 2, 255} and (patterns[-1][1] == 255).any() == (B * Nin > 8)


# ---------------------------------------------------------------------------------------------------------------- Input / LIF
def run_lif_oracle(I, kind, thresh_vec=None):
    """NODE_STEPS oracle.lif_step calls from v = rest: final state, the masked currents and both rasters.  thresh_vec: per-neuron
    thresholds, column by column through the scalar oracle (the threshold only enters the comparison of a neuron's own v)."""
    T, B, N = I.shape
    I = I.copy()
    v, r, s, x = np.full((B, N), SC.LIF_KW["rest"], f32), np.zeros((B, N), f32), np.zeros((B, N), u8), np.zeros((B, N), f32)
    ras_s, ras_v = np.zeros((T, B, N), u8), np.zeros((T, B, N), f32)
    for t in range(T):
        if thresh_vec is None:
            oracle.lif_step(v, r, s, x, I[t], **SC.LIF_KW, **kind)
        else:
            kw = dict(SC.LIF_KW)
            for j in range(N):
                col = [np.ascontiguousarray(a[:, j:j + 1]) for a in (v, r, s, x, I[t])]
                kw["thresh"] = float(thresh_vec[j])
                oracle.lif_step(*col, **kw, **kind)
                for a, c in zip((v, r, s, x, I[t]), col):
                    a[:, j:j + 1] = c
        ras_s[t], ras_v[t] = s, v
    return dict(v=v, r=r, s=s, x=x, I=I, ras_s=ras_s, ras_v=ras_v)


def lif_is_active(ref):
    """Spikes in the raster, refractory neurons whose current was masked, and a membrane sitting on lbound."""
    return bool(ref["ras_s"].any()) and bool((ref["ras_v"] == f32(SC.LIF_KW["lbound"])).any()) and bool((ref["r"] > 0).any())


@pytest.mark.parametrize("B,N", [s for s in SC.LIF_SHAPES if s[0] * s[1] <= 32768])
def test_reference_lif_spikes_and_reaches_lbound(B, N):
    """(A single neuron cannot do both within six steps: 20 mV to the threshold at 6 mV a step at most, and from the reset value it
    only decays towards rest; the activity is asserted from 255 elements on.)"""
    for kind in SC.TRACE_KINDS:
        ref = run_lif_oracle(SC.lif_currents(B, N), kind)
        assert lif_is_active(ref) == (B * N >= 255), (B, N)
    if (B, N) == (3, 257):
        th = SC.lif_thresholds(N)
        ref = run_lif_oracle(SC.lif_currents(B, N), SC.TRACE_KINDS[0], th)
        plain = run_lif_oracle(SC.lif_currents(B, N), SC.TRACE_KINDS[0])
        assert lif_is_active(ref) and (ref["ras_s"] != plain["ras_s"]).any()
        one = run_lif_oracle(SC.lif_currents(B, N), SC.TRACE_KINDS[0], np.full(N, SC.LIF_KW["thresh"], f32))
        assert all(np.array_equal(bits(one[k].astype(f32)), bits(plain[k].astype(f32))) for k in plain)     # the column form is the scalar one


def run_input_oracle(sp, kind):
    x = np.zeros(sp.shape[1:], f32)
    for t in range(sp.shape[0]):
        oracle.input_step(sp[t], x, kind["trace_decay"], kind["trace_scale"], kind["additive"])
    return x


# ---------------------------------------------------------------------------------------------------------------- Diehl&Cook
def run_dc_oracle(I, Q, one_spike=True, v0=None):
    """oracle.dc_step over the steps of I from rest with learning on: final state, the raster, the rows that drew noise per step and the
    cursor."""
    T, B, N = I.shape
    v, r, s, x = np.full((B, N), SC.DC_KW["rest"], f32), np.zeros((B, N), f32), np.zeros((B, N), u8), np.zeros((B, N), f32)
    theta, cursor = np.zeros(N, f32), np.zeros(1, np.int64)
    ras, rows = np.zeros((T, B, N), u8), []
    for t in range(T):
        rows.append(oracle.dc_step(v, r, s, x, theta, I[t], Q, cursor, learning=True, one_spike=one_spike, **SC.DC_KW))
        ras[t] = s
    return dict(v=v, r=r, s=s, x=x, theta=theta, ras=ras, rows=rows, cursor=int(cursor[0]))


def check_dc_rows(B, N, ref):
    """Every row crosses, none does, only row 0, only row B - 1 (a single row 0 = B - 1 of one neuron is still refractory then)."""
    assert ref["rows"][:3] == [B, 0, 1] and (ref["rows"][3] == 1 or (B == 1 and N == 1)), ref["rows"]
    assert ref["ras"][0].sum(1).tolist() == [1] * B and ref["ras"][2, 1:].sum() == 0 and ref["ras"][3, :B - 1].sum() == 0
    assert ref["cursor"] == sum(ref["rows"]) * N and (ref["theta"] > 0).any()


@pytest.mark.parametrize("B,N", SC.dc_shapes())
def test_reference_dc_rows_cross_as_driven(B, N):
    I, Q = SC.dc_inputs(B, N)
    ref = run_dc_oracle(I, Q)
    check_dc_rows(B, N, ref)
    assert ref["cursor"] <= Q.size
    free = run_dc_oracle(I, Q, one_spike=False)
    assert free["rows"] == [0] * SC.DC_STEPS and free["cursor"] == 0
    if N > 1:
        assert free["ras"][0].sum() > B                     # several crossings a row: the arbitration has something to decide


@pytest.mark.parametrize("lo,hi,what", SC.DC_TIES)
def test_oracle_dc_ties_go_to_the_first_maximal_index(lo, hi, what):
    I, Q = SC.dc_tie_inputs(lo, hi)
    ref = run_dc_oracle(I[None], Q)
    assert ref["rows"] == [2]
    for b in range(SC.DC_TIE_B):
        mask = torch.from_numpy((I[b] > 0).astype(f32))
        q = torch.from_numpy(Q[b * SC.DC_TIE_N:(b + 1) * SC.DC_TIE_N])
        win = int(torch.argmax(mask / q))
        assert win == lo and mask[hi] == 1 and float(q[lo]) == float(q[hi]) == float(q.min()), what
        assert ref["s"][b].nonzero()[0].tolist() == [lo], what


# ---------------------------------------------------------------------------------------------------------------- plasticity
PLASTICITY_RULES = ("postpre_dt", "postpre", "hebbian", "wdpp")


def plasticity_rates(rule, B):
    """(nu0, nu1): about 0.4 / B and 0.6 / B, so that the two batch sums (B x 0.3 x 0.5 and B x 0.5 x 0.2 on average) nearly cancel at
    every B and the weights end on both bounds and between them; Hebbian adds both sums, so its nu0 is negative."""
    nu0, nu1 = float(f32(0.4) / f32(B)), float(f32(0.6) / f32(B))
    return (-nu0 if rule == "hebbian" else nu0), nu1


def run_plasticity_oracle(rule, W, s_src, x_src, s_tgt, x_tgt, decay=SC.WDECAY):
    W = W.copy()
    nu0, nu1 = plasticity_rates(rule, s_src.shape[0])
    if rule.startswith("postpre"):
        oracle.postpre(W, s_src, x_src, s_tgt, x_tgt, nu0=nu0, nu1=nu1, use_dt=rule == "postpre_dt", dt=0.5, decay=decay, wmin=SC.WMIN, wmax=SC.WMAX)
    else:
        oracle.hebbian_wdpp(W, s_src, x_src, s_tgt, x_tgt, nu0=nu0, nu1=nu1, weight_dependent=rule == "wdpp", decay=decay, wmin=SC.WMIN,
                            wmax=SC.WMAX)
    return W


def check_bounds_and_motion(W0, W, quiet):
    """Weights on either bound, weights strictly between them that moved, and a result the spikes had a say in."""
    lo, hi = f32(SC.WMIN), f32(SC.WMAX)
    assert (W == lo).any() and (W == hi).any() and ((W > lo) & (W < hi) & (W != W0)).any() and (W != quiet).any()
    assert (W >= lo).all() and (W <= hi).all()


def run_mstdp_oracle(W, s_src, s_tgt, reward, reward_vec=None):
    """MSTDP_STEPS oracle.mstdp calls from zero traces: W after every step, the final P+ / P-."""
    T, B, Nin = s_src.shape
    N = s_tgt.shape[2]
    W = W.copy()
    elig, pp, pm = np.zeros((B, Nin, N), f32), np.zeros((B, Nin), f32), np.zeros((B, N), f32)
    Ws = []
    for t in range(T):
        oracle.mstdp(W, elig, pp, pm, s_src[t], s_tgt[t], reward=reward, reward_vec=reward_vec, wdecay=SC.WDECAY, wmin=SC.WMIN, wmax=SC.WMAX,
                     **SC.MSTDP_KW)
        Ws.append(W.copy())
    return Ws, pp, pm


MSTDPET_KW = dict(reward=0.7, nu0=0.05, dt=1.0, a_plus=1.0, a_minus=-1.0, decay_plus=SC.MSTDP_KW["decay_plus"],
                  decay_minus=SC.MSTDP_KW["decay_minus"], decay_e=float(np.exp(f32(-1.0 / 25.0))), tc_e=25.0)


def run_mstdpet_oracle(W, s_src, s_tgt):
    """s_src [T, Nin], s_tgt [T, N] (batch 1): W and the eligibility trace after every step, the final P+ / P-."""
    T, Nin = s_src.shape
    N = s_tgt.shape[1]
    W = W.copy()
    elig, et, pp, pm = np.zeros((Nin, N), f32), np.zeros((Nin, N), f32), np.zeros(Nin, f32), np.zeros(N, f32)
    out = []
    for t in range(T):
        oracle.mstdpet(W, elig, et, pp, pm, s_src[t], s_tgt[t], wdecay=SC.WDECAY, wmin=SC.WMIN, wmax=SC.WMAX, **MSTDPET_KW)
        out.append((W.copy(), et.copy()))
    return out, pp, pm


def check_mstdpet_activity(W0, steps):
    """A non-zero eligibility trace, weights held on wmin, weights clamped to wmax by the first step (the decay of 0.99 takes them off it
    again: the trace moves a weight by far less than one percent a step), and weights between the bounds that the spikes moved."""
    lo, hi = f32(SC.WMIN), f32(SC.WMAX)
    Nin, N = W0.shape
    quiet, _, _ = run_mstdpet_oracle(W0, np.zeros((len(steps), Nin), u8), np.zeros((len(steps), N), u8))
    (W1, _), (W, et) = steps[0], steps[-1]
    assert (et != 0).any() and (W == lo).any() and (W1 == hi).any()
    assert ((W > lo) & (W < hi) & (W != quiet[-1][0])).any()


def test_reference_mstdpet_is_active_beyond_the_grid_cap():
    Nin, N = SC.MSTDPET_CAP
    W, s_src, s_tgt, _ = SC.mstdp_inputs(1, Nin, N)
    steps, pp, pm = run_mstdpet_oracle(W, s_src[:, 0], s_tgt[:, 0])
    check_mstdpet_activity(W, steps)
    assert (pp != 0).any() and (pm != 0).any()


@pytest.mark.parametrize("B", sorted(SC.PLASTICITY_B))
def test_reference_plasticity_reaches_both_bounds_and_moves(B):
    for shape in SC.plasticity_shapes(B):
        W0, s_src, x_src, s_tgt, x_tgt = SC.plasticity_inputs(*shape)
        z_src, z_tgt = np.zeros_like(s_src), np.zeros_like(s_tgt)
        for rule in PLASTICITY_RULES:
            check_bounds_and_motion(W0, run_plasticity_oracle(rule, W0, s_src, x_src, s_tgt, x_tgt),
                                    run_plasticity_oracle(rule, W0, z_src, x_src, z_tgt, x_tgt))
        Wi, q_src, _, q_tgt, _ = SC.plasticity_inputs(*shape, inside=True, sparse=True)
        assert (Wi >= f32(SC.WMIN)).all() and (Wi <= f32(SC.WMAX)).all()
        assert q_src.any() and q_tgt.any() and not q_src.any(0).all() and not q_tgt.any(0).all()          # silent rows and columns to skip
        W, s_src, s_tgt, rv = SC.mstdp_inputs(*shape)
        for reward, vec in ((0.7, None), (0.0, rv)):
            Ws, pp, pm = run_mstdp_oracle(W, s_src, s_tgt, reward, vec)
            quiet, _, _ = run_mstdp_oracle(W, np.zeros_like(s_src), np.zeros_like(s_tgt), reward, vec)
            check_bounds_and_motion(W, Ws[-1], quiet[-1])
